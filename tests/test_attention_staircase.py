"""CPU: the construction of the threshold staircase (tests/attention_staircase.py) that tests/test_gpu_attention_exact.py runs through
the attention kernels — what places each case on the intended side of a lazy-rescale threshold."""
import numpy as np
import pytest

from attention_staircase import N_TILES, STAIR_K, TILE, staircase


@pytest.mark.parametrize("dk", [128, 80])
@pytest.mark.parametrize("step", [9.5, 10.5, 15.5, 16.5])
def test_staircase_construction(step, dk):
    """In fp64, on the fp32 inputs: query 1's base-2 score on key 32 t + 5 is step * t in every tile t, and from tile 1 on that score
    IS the tile's maximum (the planted score of tile 0 is 0: its maximum is a random key, a few units), so the per-tile maximum rises
    by `step` base-2 units from tile to tile — all within 1e-3."""
    Q, K, _ = staircase(step, dk, 2)
    s2 = (Q[1, :dk].astype(np.float64) @ K[:, :dk].astype(np.float64).T) * dk ** -0.5 / np.log(2.0)
    tile_max = np.array([s2[TILE * t:TILE * (t + 1)].max() for t in range(N_TILES)])
    planted = s2[5::TILE]
    assert N_TILES == 10 and planted.shape == (N_TILES,)
    assert np.abs(planted - step * np.arange(N_TILES)).max() < 1e-3
    assert np.array_equal(tile_max[1:], planted[1:])                         # the planted key is the tile's maximum from tile 1 on
    assert np.abs(np.diff(tile_max[1:]) - step).max() < 1e-3                 # ... which rises by `step` per tile
    assert abs((tile_max[1] - planted[0]) - step) < 1e-3
    other = np.delete(s2, np.arange(5, STAIR_K, TILE))
    assert 0 < tile_max[0] == other[:TILE - 1].max() and np.abs(other).max() < 8.0     # random keys: never near the first planted step
