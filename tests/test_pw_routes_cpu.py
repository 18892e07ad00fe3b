"""Pointwise routes: every host-only query of csrc/pwconv.hip, pwfused.hip and bf16.hip answers the fixed shape list of
tests/golden/make_pw_routes.py exactly as tests/golden/pw_routes.npz recorded it before the host code got its single route
(csrc/pwroute.hpp).  Which kernel a shape takes and how many partials or slabs it writes is pinned; host arithmetic only (CPU)."""
import numpy as np

from mslesions3d_amd import _lib
from tests import pw_cases as C
from tests.golden import make_pw_routes as R


def test_route_table_covers_the_list():
    z = np.load(R.OUT)
    shapes = R.shapes()
    assert z["shapes"].dtype == np.int32 and z["answers"].dtype == np.int64
    assert z["shapes"].tolist() == [list(s) for s in shapes], "tests/golden/pw_routes.npz was minted for another shape list"
    assert z["answers"].shape == (len(shapes), len(R.COLUMNS))
    assert len(shapes) >= 2000
    for name in R.COUNTING:
        assert len(np.unique(z["answers"][:, R.COLUMNS.index(name)])) >= 6, name
    assert int((z["answers"][:, R.COLUMNS.index("msl_pwconv_bwd_fused_num_partials")] != 0).sum()) >= 100


def test_pointwise_queries_answer_as_recorded():
    z = np.load(R.OUT)
    got = R.answers(_lib.load(), [tuple(s) for s in z["shapes"].tolist()])
    want = z["answers"]
    bad = np.argwhere(got != want)
    assert bad.size == 0, "; ".join(
        f"{R.COLUMNS[j]}{tuple(z['shapes'][i].tolist())} = {got[i, j]}, recorded {want[i, j]}" for i, j in bad[:8].tolist())


def test_the_list_reaches_every_kind():
    """A condition on the list, not on the code: at least 50 shapes of it reach each PwKind other than None."""
    L = _lib.load()
    count = dict.fromkeys(range(1, len(C.KIND)), 0)
    for n, cin, cout, s in R.shapes():
        kinds = {L.msl_pwconv_route_kind(op, bf16, n, cin, cout, s, 1) for op in range(4) for bf16 in (0, 1)}
        for k in kinds - {0}:
            count[k] += 1
    assert all(v >= 50 for v in count.values()), count
