"""The threshold staircase of the lazy-rescale tests (tests/test_gpu_attention_exact.py; its construction is checked on the CPU by
tests/test_attention_staircase.py): one attention segment in which ONE query's running maximum climbs by a fixed number of base-2
units per 32-key tile, so that it lands just below or just above the kernels' rescale thresholds, tile after tile."""
import numpy as np

STAIR_Q, STAIR_K, TILE = 70, 300, 32
N_TILES = (STAIR_K + TILE - 1) // TILE


def staircase(step, dk, n_head, seed=7):
    """70 queries x 300 keys of N(0,1) where, in every 32-key tile t, key 32 t + 5 of head 0 is q1 * target_t / (scale * q1.q1): query
    1's base-2 score on that key is step * t.  From tile 1 on that key is its tile's maximum, so query 1's maximum climbs by `step`
    per tile and lands just below (9.5, 15.5) or just above (10.5, 16.5) the rescale threshold (m_run + 10, m_run + 16) relative to
    the tile at which the reference last moved.  The other 31 queries of its wave stay random."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((STAIR_Q, n_head * dk)).astype(np.float32)
    K = rng.standard_normal((STAIR_K, n_head * dk)).astype(np.float32)
    V = rng.standard_normal((STAIR_K, n_head * dk)).astype(np.float32)
    q1 = Q[1, :dk].astype(np.float64)
    scale = dk ** -0.5
    for t in range(N_TILES):
        target = step * t * np.log(2.0)                          # natural-log units: base-2 score step * t
        K[TILE * t + 5, :dk] = (q1 * (target / (scale * (q1 @ q1)))).astype(np.float32)
    return Q, K, V
