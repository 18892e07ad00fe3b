import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# torch's CPU log / exp run through MKL, whose default code path is picked per CPU vendor and ISA and differs in the last
# ulp between hosts.  The fixtures under tests/golden/ were minted on MKL's vendor-independent path (make_golden.py):
# take the same one here, before the first MKL call, so that the bit-exact oracle tests hold on any x86 host.
os.environ["MKL_CBWR"] = "COMPATIBLE"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with `-m gpu` on the GPU box)")


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)
