"""The two host-side tables behind the ragged batch build (devicedata.py): ``pack_launch``, the one f64 upload of a
launch, and ``RESAMPLERS``, the resampling transforms ``sample_params`` knows by name."""
import numpy as np
import pytest

from mslesions3d_amd import datasets as DS
from mslesions3d_amd.devicedata import AFFINE_STRIDE, BOUNDARY, RESAMPLERS, pack_launch, sample_params


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("with_windows", [False, True])
@pytest.mark.parametrize("with_table", [False, True])
def test_pack_launch_layout(with_table, with_windows, N):
    """Rows, then the f64 table, then the int32 origins in the doubles behind them, at the offsets returned."""
    rs = np.random.RandomState(7 * N + 2 * with_table + with_windows)
    rows = rs.randn(N, AFFINE_STRIDE)
    table = rs.randn(11) if with_table else np.zeros(0)
    windows = [tuple(int(v) for v in rs.randint(-40, 40, 3)) for _ in range(N)] if with_windows else None
    packed, at_table, at_windows = pack_launch(rows, table, windows)
    n_int = 3 * N if with_windows else 0
    assert packed.dtype == np.float64 and packed.ndim == 1 and packed.flags["C_CONTIGUOUS"]
    assert packed.size == rows.size + table.size + (n_int + 1) // 2
    assert (at_table, at_windows) == (rows.size, rows.size + table.size)
    assert np.array_equal(packed[:at_table], rows.reshape(-1))
    assert np.array_equal(packed[at_table:at_windows], table)
    tail = packed[at_windows:].view(np.int32)
    if with_windows:
        assert np.array_equal(tail[:3 * N], np.asarray(windows, dtype=np.int32).reshape(-1))
    if with_windows and N % 2:
        assert tail.size == 3 * N + 1 and tail[-1] == 0
    else:
        assert tail.size == n_int
    if not with_table and not with_windows:  # the fit's upload is the rows themselves
        assert packed.tobytes() == rows.reshape(-1).tobytes()


AFTER_AN_OPERATION = {"affine": "device pipeline: an affine stage after an intensity operation",
                      "zoom": "device pipeline: a warp stage after an intensity operation",
                      "griddistortion": "device pipeline: a warp stage after an intensity operation",
                      "elastic3d": "device pipeline: a deformation stage after an intensity operation"}
ON_THE_EXAMPLE_CACHE = {"zoom": "device pipeline: zoom / griddistortion on the example cache",
                        "griddistortion": "device pipeline: zoom / griddistortion on the example cache",
                        "elastic3d": "device pipeline: elastic3d on the example cache"}


def test_the_table_names_the_resampling_transforms():
    assert set(RESAMPLERS) == set(AFTER_AN_OPERATION)
    assert {n for n, r in RESAMPLERS.items() if r.ragged_only} == set(ON_THE_EXAMPLE_CACHE)


@pytest.mark.parametrize("name", sorted(AFTER_AN_OPERATION))
def test_every_resampler_of_the_table_through_sample_params(name):
    shape = (9, 11, 10)
    augs = [(name, {"prob": 1.0})]
    draws = DS.draw_augmentations(augs, np.random.RandomState(3))
    assert draws[0][1] is not None
    _, stages = sample_params(draws, shape, augs, ragged=True)
    assert len(stages) == 1 and type(stages[0]) is RESAMPLERS[name].stage
    assert stages[0].boundary == BOUNDARY[RESAMPLERS[name].pad]  # the entry names no padding_mode
    assert sample_params([(name, None)], shape, augs, ragged=True)[1] == [None]
    with pytest.raises(NotImplementedError) as e:
        sample_params([("shiftintensity", None), (name, None)], shape, ragged=True)
    assert str(e.value) == AFTER_AN_OPERATION[name]
    if name in ON_THE_EXAMPLE_CACHE:
        with pytest.raises(NotImplementedError) as e:
            sample_params([(name, None)], shape)
        assert str(e.value) == ON_THE_EXAMPLE_CACHE[name]
    else:
        assert sample_params([(name, None)], shape)[1] == [None]
