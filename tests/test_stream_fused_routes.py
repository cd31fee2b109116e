"""CPU: the case table of tests/stream_fused_cases.py reaches every route the one-window fused launchers (csrc/stream_fused.hip)
can take — for the served models' launches and for a grid across every threshold of the dispatch.  The routes come from the
launchers' own route functions (no device needed), so a new instantiation or a moved threshold that no case reaches fails here."""
import importlib
import os

import pytest

import stream_fused_cases as T


@pytest.fixture(scope="module")
def ops(pkg):
    set_knobs = [k for k in T.KNOBS if k in os.environ]
    if set_knobs:
        pytest.fail(f"{set_knobs} change the dispatch under test: unset them")
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return importlib.import_module("asr_2pass_amd.ops")


def test_every_case_takes_the_route_it_is_listed_under(ops):
    """At both ends of its row range, and at 1 / 5 / 6 / 20 rows nowhere else than the table says."""
    wrong = []
    for c in T.CASES:
        for M in (c.m_lo, c.m_hi):
            got = T.route_of(ops, c.form, M, c.N, c.K, c.ln, c.fsmn)
            if got != c.route:
                wrong.append((c, M, got))
    assert not wrong, wrong[:10]
    assert len({c.route for c in T.REPRESENTATIVES}) == len(T.REPRESENTATIVES)


def test_representatives_are_what_the_route_functions_generate(ops):
    assert T.REPRESENTATIVES == T.representatives(ops), "regenerate: python tests/stream_fused_cases.py"


def test_table_reaches_every_route_of_the_served_models(ops, weights_mod):
    have = {c.route for c in T.CASES}
    grid = T.production_grid(ops, weights_mod)
    assert len(grid) == 2 * 32 * 12 - 2 * 12       # every call at every row count; the predictor conv above 20 rows is the general GEMM's
    missing = sorted({g for g in grid if g[-1] not in have}, key=lambda g: g[-1])
    assert not missing, f"routes of served shapes that no case runs: {missing[:10]}"


def test_table_reaches_every_route_of_the_reachable_grid(ops):
    have = {c.route for c in T.CASES}
    missing = {}
    for g in T.reachable_grid(ops):
        if g[-1] not in have:
            missing.setdefault(g[-1], g)
    assert not missing, f"{len(missing)} routes that no case runs, e.g. {sorted(missing.values(), key=lambda g: g[-1])[:10]}"


def test_known_routes(ops):
    """The served shapes whose dispatch a refactor must not move."""
    r1, rl = ops.fused_gemv_1trip_route, ops.fused_ln_gemm_route
    # predictor conv of the large model
    assert r1(20, 512, 1536) == dict(ok=True, ln=False, fs=False, cw=4, cpl=2, rpl=5, nf=3, waves=16)
    # the small model's FFN2 / folded decoder FFN2: Chan's merge over 10 waves; K = 320 and 960 give 5 and 15
    assert r1(20, 320, 1280, ln=True) == dict(ok=True, ln=True, fs=False, cw=4, cpl=2, rpl=5, nf=4, waves=10)
    assert r1(20, 320, 320, ln=True)["waves"] == 5 and r1(20, 320, 960, ln=True)["waves"] == 15
    # the small model's QKV / FFN1: 20 waves, refused; then the vector form on 8 columns, 10 k-blocks
    for ln in (False, True):
        assert not r1(20, 960, 320, ln=ln)["ok"]
        assert rl(20, 960, 320, ln=ln) == dict(kernel="vector", ln=ln, cw=8, mr=24, waves=16 if ln else 10, k_blocks=10)
    # a decoder window above 20 tokens
    assert not r1(21, 512, 512)["ok"] and r1(20, 512, 512)["ok"]
    assert rl(25, 512, 2048, ln=True) == dict(kernel="vector", ln=True, cw=2, mr=32, waves=16, k_blocks=16)
    # the vocabulary projection
    assert rl(20, 8404, 512, ln=True) == dict(kernel="matrix", ln=True, cw=32, mr=32, waves=16, k_blocks=64)
    # the one-trip form takes no LayerNorm together with the FSMN memory
    assert not r1(20, 512, 512, ln=True, fsmn=True)["ok"]
    assert r1(8, 512, 512, fsmn=True) == dict(ok=True, ln=False, fs=True, cw=4, cpl=2, rpl=2, nf=2, waves=8)
    # the large model's FFN2 and the first layer's padded K
    assert r1(20, 512, 2048) == dict(ok=True, ln=False, fs=False, cw=2, cpl=2, rpl=5, nf=2, waves=16)
    assert rl(20, 1536, 576, ln=True) == dict(kernel="vector", ln=True, cw=8, mr=24, waves=16, k_blocks=18)


def test_vector_form_never_leaves_a_tail_of_k_or_an_output_without_a_thread(ops):
    """What the table found: with 2-column patches the k-block is 128, so K % 128 == 64 dropped the last 64 columns; and K = 64
    without LayerNorm ran fewer threads than the MR x CW outputs of a workgroup.  Over the whole grid: the k-blocks of the vector
    form cover K exactly, and the threads cover the outputs."""
    assert ops.fused_ln_gemm_route(20, 512, 1088)["cw"] == 4
    for N in T.GRID_N:
        for K in T.GRID_K:
            for M in T.GRID_M:
                r = ops.fused_ln_gemm_route(M, N, K)
                if r["kernel"] == "vector":
                    assert r["k_blocks"] * (256 // r["cw"]) == K, (M, N, K, r)
                    assert 64 * r["waves"] >= r["mr"] * r["cw"], (M, N, K, r)


def test_route_entries_refuse_what_the_operator_refuses(ops):
    with pytest.raises(Exception):
        ops.fused_ln_gemm_route(33, 512, 512)
    with pytest.raises(Exception):
        ops.fused_ln_gemm_route(20, 512, 100)
