"""Depthwise routes: every host-only query of csrc/dwconv.hip, dwconv_bwd.hip and bf16.hip answers the fixed shape list of
tests/golden/make_dw_routes.py exactly as tests/golden/dw_routes.npz recorded it before the host code got its single route
(csrc/dwroute.hpp).  Which kernel a shape takes and how many partials it writes is pinned; host arithmetic only (CPU)."""
import numpy as np

from mslesions3d_amd import _lib
from tests.golden import make_dw_routes as R


def test_route_table_covers_the_list():
    z = np.load(R.OUT)
    shapes = R.shapes()
    assert z["shapes"].dtype == np.int32 and z["answers"].dtype == np.int32
    assert z["shapes"].tolist() == [list(s) for s in shapes], "tests/golden/dw_routes.npz was minted for another shape list"
    assert z["answers"].shape == (len(shapes), len(R.QUERIES))
    assert len(shapes) >= 2000
    variants = z["answers"][:, 0].tolist()
    assert all(variants.count(v) >= 100 for v in (0, 1, 2, 3))  # naive, stream, resident, wave


def test_depthwise_queries_answer_as_recorded():
    z = np.load(R.OUT)
    got = R.answers(_lib.load(), [tuple(s) for s in z["shapes"].tolist()])
    want = z["answers"]
    bad = np.argwhere(got != want)
    assert bad.size == 0, "; ".join(
        f"{R.QUERIES[j][0]}{tuple(z['shapes'][i].tolist())} = {got[i, j]}, recorded {want[i, j]}" for i, j in bad[:8].tolist())
