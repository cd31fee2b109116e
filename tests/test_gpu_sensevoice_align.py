"""GPU: CTC forced alignment at the model level (pfhip_svs_align) on test_gpu_sensevoice.py's small synthetic model.

"The greedy tokens" of an utterance are here the collapse of its SPEECH rows, R.ctc_collapse(frame_ids[4:]): in a trained model the
four prompt rows emit exactly the four tags, so that is ids[4:]; the synthetic weights put blanks and repeats into the prompt rows,
and ids[4:] would cut at the wrong place.

Bounds.  eps = max |E_gpu - E_ref| over the gathered entries, asserted below LOGP_TOL = 1e-3, the bound test_gpu_sensevoice.py holds
for frame_logp.  A path that is optimal under emissions which are off by at most eps per frame loses at most 2 N eps on the exact
emissions (N eps on its own score, N eps on the rival's), so the GPU path scored on E_ref must be within 2 N eps of the restatement's
optimum on E_ref; and where every frame's top-2 gap in E_ref exceeds 2 N eps the greedy path is the only optimum under both."""
import ctypes
import functools
import importlib
import threading

import numpy as np
import pytest

import ctc_align_ref as ref
import sensevoice_ref as R
import test_gpu_sensevoice as SV
from oracle import paraformer as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LOGP_TOL = SV.LOGP_TOL
SECONDS, LIDS, TEXTNORMS = SV.SECONDS, SV.LIDS, SV.TEXTNORMS
D, BLANK = 512, 0


@pytest.fixture(scope="module")
def ops(pkg):
    return importlib.import_module("asr_2pass_amd.ops")


@pytest.fixture(scope="module")
def model(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    m = pkg.SenseVoiceHip().InitAsr(SV.container(), device=0)
    yield m
    m.close()


def forward(model):
    return model.forward(SV.packed(), lid=LIDS, textnorm=TEXTNORMS)


def greedy_tokens(got):
    return [R.ctc_collapse(f[4:], BLANK)[0] if len(f) else [] for f in got["frame_ids"]]


def thinned(tokens):
    return [[t for i, t in enumerate(y) if i % 3 != 2] for y in tokens]


@functools.lru_cache(maxsize=None)
def e_ref(b, tokens):
    """The oracle's emissions of blank | tokens over the speech rows of utterance b, float64."""
    lp = SV.reference(b, SECONDS[b], LIDS[b], TEXTNORMS[b])["logp"]
    return lp[4:][:, [BLANK] + list(tokens)].astype(np.float64)


def gpu_emissions(model, ops, got, tokens):
    """(E per utterance, spans of ops.ctc_align, lse) from what the forward left: get_tensor("enc"), the container's ctc.w / ctc.b
    and get_tensor("lse"), the rows' log-sum-exp as the CTC head that ran kept it (the fused head's merge kernel, or the unfused
    head's row kernel)."""
    rows = [int(n) for n in got["frame_len"]]
    M = sum(rows)
    w = P.Weights(*SV.container())
    enc = torch.from_numpy(model.get_tensor("enc", M * D).reshape(M, D).copy()).cuda()
    lse_h = model.get_tensor("lse", M).copy()
    assert lse_h.shape == (M,)
    lse = torch.from_numpy(lse_h).cuda()
    Wd, bd = torch.from_numpy(np.array(w["ctc.w"], np.float32)).cuda(), torch.from_numpy(np.array(w["ctc.b"], np.float32)).cuda()
    row_off = np.concatenate([[0], np.cumsum(rows)])[:-1]
    lab = ops.CtcLabels(tokens, [max(r - 4, 0) for r in rows])
    E = ops.ctc_emissions(enc, Wd, bd, lse, torch.tensor((row_off + 4).tolist(), dtype=torch.int32, device="cuda"), lab, blank=BLANK)
    tb, te, tl, sc = ops.ctc_align(E, lab)
    torch.cuda.synchronize()
    Eh = E.cpu().numpy()
    return [lab.cut(Eh, b) for b in range(lab.B)], tb.cpu().numpy(), te.cpu().numpy(), tl.cpu().numpy(), sc.cpu().numpy(), lse_h


def lse_ref(b):
    """float64 log-sum-exp of every row of utterance b, from the oracle's rows after tp.norm."""
    w = P.Weights(*SV.container())
    enc = SV.reference(b, SECONDS[b], LIDS[b], TEXTNORMS[b])["enc"]
    logits = enc.astype(np.float64) @ np.asarray(w["ctc.w"], np.float64).T + np.asarray(w["ctc.b"], np.float64)
    m = logits.max(axis=1)
    return m + np.log(np.exp(logits - m[:, None]).sum(axis=1))


def check_wiring(al, tokens, tb, te, tl, sc):
    """pfhip_svs_align == ops.ctc_emissions + ops.ctc_align on what the forward kept, bit for bit."""
    assert al["score"].tobytes() == sc.tobytes()
    for b, y in enumerate(tokens):
        L = len(y)
        assert al["begin"][b].tolist() == (tb[b, :L] + 4).tolist() and al["end"][b].tolist() == (te[b, :L] + 4).tolist()
        assert al["logp"][b].tobytes() == tl[b, :L].tobytes()


def check_optimal(model, ops, got, tokens, what):
    """Points 1, 2 and 3 for one token set on whatever head the last forward took; returns (eps, spans).  E_gpu are the emissions
    the aligner itself used: check_wiring holds pfhip_svs_align to them bit for bit."""
    al = model.align(tokens)
    Es, tb, te, tl, sc, lse = gpu_emissions(model, ops, got, tokens)
    check_wiring(al, tokens, tb, te, tl, sc)
    eps, e_lse, r0 = 0.0, 0.0, 0
    for b in range(len(tokens)):
        rows = int(got["frame_len"][b])
        if rows:
            eps = max(eps, float(np.abs(Es[b] - e_ref(b, tuple(tokens[b]))).max()))          # every gathered entry
            e_lse = max(e_lse, float(np.abs(lse[r0:r0 + rows] - lse_ref(b)).max()))           # every row, prompt rows included
        r0 += rows
    print(f"{what}: eps = max |E_gpu - E_ref| = {eps:.3e}, max |lse_gpu - lse_ref| = {e_lse:.3e} (bound {LOGP_TOL:.0e})")
    assert eps < LOGP_TOL and e_lse < LOGP_TOL
    for b in range(1, len(tokens)):
        rows, y = int(got["frame_len"][b]), tokens[b]
        N, Er = rows - 4, e_ref(b, tuple(tokens[b]))
        begin, end, logp = al["begin"][b], al["end"][b], al["logp"][b]
        assert np.isfinite(al["score"][b])
        # structure: ordered, disjoint, inside [4, rows), non-empty
        assert (begin >= 4).all() and (end <= rows).all() and (begin < end).all()
        assert (begin[1:] >= end[:-1]).all()
        for j in range(len(y) - 1):
            if y[j] == y[j + 1]:
                assert begin[j + 1] > end[j]                         # a blank between equal neighbours
        path = ref.path_from_spans(N, begin - 4, end - 4)
        assert path[0] <= 1 and path[-1] >= 2 * len(y) - 1
        assert ref.collapse(path, y) == y
        # tok_logp is the forward's log-prob entry of that token at that row
        assert np.abs(logp - Er[begin - 4, np.arange(len(y)) + 1]).max() <= eps if len(y) else True
        # the score is the restatement's on the emissions the aligner used, bit for bit
        assert np.float32(al["score"][b]).tobytes() == np.float32(ref.viterbi(Es[b], y)[0]).tobytes()
        # optimality on the reference emissions: the optimum in float64, the GPU's path and score within 2 N eps of it
        best = float(ref.viterbi(Er, y, dtype=np.float64)[0])
        mine = ref.path_score(Er, path)
        print(f"{what}, utterance {b}: N {N}, L {len(y)}, optimum on E_ref {best:.6f}, GPU path on E_ref {mine:.6f}, "
              f"GPU score {float(al['score'][b]):.6f}, 2 N eps {2 * N * eps:.3e}")
        assert mine <= best + 1e-9 and best - mine <= 2 * N * eps
        assert abs(float(al["score"][b]) - best) <= 2 * N * eps
    return eps, al


def test_wiring_is_exact(model, ops):
    """pfhip_svs_align == ops.ctc_emissions fed with get_tensor("enc"), the container's ctc.w / ctc.b and the forward's own row
    log-sum-exp, followed by ops.ctc_align: the offset of 4, the blank id, the label gather."""
    got = forward(model)
    for tokens in (greedy_tokens(got), thinned(greedy_tokens(got))):
        al = model.align(tokens)
        Es, tb, te, tl, sc, lse = gpu_emissions(model, ops, got, tokens)
        check_wiring(al, tokens, tb, te, tl, sc)
        for b, y in enumerate(tokens):
            if y and int(got["frame_len"][b]):
                # that log-sum-exp is the forward's: the emission at a greedy frame is that frame's log-prob
                f = got["frame_ids"][b]
                for j in range(len(y)):
                    t = int(al["begin"][b][j])
                    if int(f[t]) == y[j]:
                        assert abs(float(al["logp"][b][j]) - float(got["frame_logp"][b][t])) < 1e-5
        assert sum(len(y) for y in tokens) > 20


def test_optimal_against_the_reference(model, ops):
    got = forward(model)
    tokens = greedy_tokens(got)
    check_optimal(model, ops, got, tokens, "greedy tokens")
    check_optimal(model, ops, got, thinned(tokens), "every third token removed")


def test_greedy_spans_are_the_runs_of_the_frame_ids(model, ops):
    got = forward(model)
    tokens = greedy_tokens(got)
    eps, al = check_optimal(model, ops, got, tokens, "greedy tokens")
    forced = []
    for b in range(1, len(tokens)):
        r = SV.reference(b, SECONDS[b], LIDS[b], TEXTNORMS[b])
        lp = np.sort(r["logp"][4:], axis=1)
        N = lp.shape[0]
        if float((lp[:, -1] - lp[:, -2]).min()) > 2 * N * eps and got["frame_ids"][b].tolist() == [int(x) for x in r["frame_ids"]]:
            forced.append(b)
    print(f"greedy spans forced in {len(forced)} of {len(tokens) - 1} utterances with rows: {forced}")
    assert forced, "no utterance has every top-2 gap above 2 N eps: the test shows nothing"
    for b in forced:
        f = got["frame_ids"][b][4:]
        begin, end = [], []
        for t in range(len(f)):
            if f[t] != BLANK and (t == 0 or f[t] != f[t - 1]):
                begin.append(t + 4)
            if f[t] != BLANK and (t + 1 == len(f) or f[t + 1] != f[t]):
                end.append(t + 5)
        assert al["begin"][b].tolist() == begin and al["end"][b].tolist() == end


def test_entry_point_behaviour(model, pkg, weights_mod):
    got = forward(model)
    tokens = greedy_tokens(got)
    B = len(tokens)
    # too many tokens for the rows: one token doubled until N < L + equal neighbours
    b = 2
    N = int(got["frame_len"][b]) - 4
    y = list(tokens[b])
    while ref.feasible(N, y):
        y.append(y[-1])
    al = model.align([tokens[i] if i != b else y for i in range(B)])
    assert al["score"][b] == -np.inf and (al["begin"][b] == -1).all() and (al["end"][b] == -1).all()
    base = model.align(tokens)
    for i in range(B):
        if i != b:                                                   # the others are served, and as without it
            assert al["score"][i].tobytes() == base["score"][i].tobytes() and al["begin"][i].tolist() == base["begin"][i].tolist()
    # utterance 0 has 320 samples: no rows.  No tokens: score 0; any token: infeasible
    assert int(got["frame_len"][0]) == 0 and base["score"][0] == 0.0
    al = model.align([[5]] + tokens[1:])
    assert al["score"][0] == -np.inf and al["begin"][0].tolist() == [-1]
    # refused before any launch
    for bad in ([BLANK], [1003], [-1]):
        with pytest.raises(pkg.PfhipError) as e:
            model.align([tokens[1] + bad] + tokens[1:])
        assert e.value.status == 1
    with pytest.raises(pkg.PfhipError) as e:
        model.align(tokens[:-1])                                     # batch mismatch
    assert e.value.status == 1
    with pytest.raises(pkg.PfhipError) as e:
        model.align(tokens, max_tokens=max(len(y) for y in tokens) - 1)
    assert e.value.status == 5                                       # PFHIP_ERR_CAPACITY
    fresh = pkg.SenseVoiceHip().InitAsr(SV.container(), device=0)
    try:
        with pytest.raises(pkg.PfhipError) as e:
            fresh.align(tokens)                                      # this handle has run no forward
        assert e.value.status == 1
        # the note of "my last forward" is per handle: a forward on another handle does not take this one's away
        fresh.forward(SV.packed()[1:3])
        again = model.align(tokens)
        assert again["score"].tobytes() == base["score"].tobytes()
        assert [x.tolist() for x in again["begin"]] == [x.tolist() for x in base["begin"]]
    finally:
        fresh.close()
    cfg = weights_mod.small_config(enc_layers=1, dec_layers=1)
    para = pkg.ParaformerHip().InitAsr(weights_mod.synth_weights(cfg), device=0)
    try:
        sv = pkg.SenseVoiceHip()
        sv._h = para._h
        try:
            with pytest.raises(pkg.PfhipError) as e:
                sv.align([[5]])
            assert e.value.status == 4                               # PFHIP_ERR_UNSUPPORTED
        finally:
            sv._h = ctypes.c_void_p()
    finally:
        para.close()


def same_forward(a, b):
    for k in ("token_num", "frame_len"):
        assert a[k].tobytes() == b[k].tobytes()
    for k in ("ids", "tok_frame", "tok_logp", "frame_ids", "frame_logp"):
        for x, y in zip(a[k], b[k]):
            assert x.tobytes() == y.tobytes(), k


def test_forward_is_unchanged_and_the_unfused_head_aligns_too(model, ops):
    """A forward after an align returns the bits it returned before.  A forward on the unfused head keeps its own log-sum-exp (the
    row kernel over each chunk's logits): it is within the model bound of float64 on every row, the emissions the aligner forms with
    it are within eps of E_ref on every gathered entry, and path and score meet the bounds of point 2 with that eps."""
    a = forward(model)
    tokens = greedy_tokens(a)
    eps_fused, fused = check_optimal(model, ops, a, tokens, "fused head, greedy tokens")
    fused_lse = model.get_tensor("lse", int(a["frame_len"].sum())).copy()
    same_forward(a, forward(model))
    before = model.debug_poke("ctc_unfused_forwards")
    assert model.debug_poke("ctc_unfused", 1) == 0
    u = forward(model)
    assert model.debug_poke("ctc_unfused_forwards") == before + 1
    assert greedy_tokens(u) == tokens
    unfused_lse = model.get_tensor("lse", int(u["frame_len"].sum())).copy()
    print(f"log-sum-exp, unfused against fused head: max abs difference {float(np.abs(unfused_lse - fused_lse).max()):.3e}")
    eps, al = check_optimal(model, ops, u, tokens, "unfused head, greedy tokens")
    check_optimal(model, ops, u, thinned(tokens), "unfused head, every third token removed")
    for b in range(1, len(tokens)):
        N = int(u["frame_len"][b]) - 4
        assert abs(float(al["score"][b]) - float(fused["score"][b])) <= 2 * N * (eps + eps_fused)      # each within 2 N eps of the same optimum


def test_unfused_head_keeps_the_log_sum_exp_of_every_chunk(model):
    """8 x 27 s = 3632 rows are two chunks of the unfused head (2048 rows each): the log-sum-exp it keeps lands on the right rows of
    both.  Both heads' values are within the model bound of the float64 value (check_optimal asserts that on the small pack), so
    they are within twice that of each other; rows of a wrong chunk would be off by the spread of the rows' log-sum-exp, ~0.1 - 1."""
    utts = [SV.utterance(10 + i, 27.0) for i in range(8)]
    f = model.forward(utts, lid=SV.PLANE_LIDS, textnorm=SV.PLANE_TEXTNORMS)
    M = int(f["frame_len"].sum())
    assert M == 3632
    fused_lse = model.get_tensor("lse", M).copy()
    assert model.debug_poke("ctc_unfused", 1) == 0
    u = model.forward(utts, lid=SV.PLANE_LIDS, textnorm=SV.PLANE_TEXTNORMS)
    assert model.debug_poke("ctc_head_chunks") == 2
    unfused_lse = model.get_tensor("lse", M).copy()
    d = np.abs(unfused_lse - fused_lse)
    print(f"3632 rows, two chunks: max |lse unfused - lse fused| = {float(d.max()):.3e}, spread of lse {float(np.ptp(fused_lse)):.3e}")
    assert np.isfinite(unfused_lse).all() and float(d.max()) < 2 * LOGP_TOL and float(np.ptp(fused_lse)) > 20 * LOGP_TOL
    al = model.align(greedy_tokens(u))
    assert np.isfinite(al["score"]).all() and all((b >= 4).all() for b in al["begin"])


def test_rows_taken_by_another_threads_forward_are_refused(model, pkg):
    """One execution context: a forward of another thread replaces the rows this thread's forward left, and align says so
    (PFHIP_ERR_ARG) instead of aligning this thread's tokens against that thread's rows — also when the batch sizes agree."""
    got = forward(model)
    tokens = greedy_tokens(got)
    other = threading.Thread(target=forward, args=(model,))
    other.start()
    other.join()
    with pytest.raises(pkg.PfhipError) as e:
        model.align(tokens)
    assert e.value.status == 1
    forward(model)
    assert np.isfinite(model.align(tokens)["score"][1:]).all()        # this thread's own forward again: served


def test_each_thread_aligns_its_own_forward(model):
    batches = [([1, 2, 3], None), ([4, 5], None)]
    utts = lambda idx: [SV.utterance(i, SECONDS[i]) for i in idx]
    want = []
    for idx, _ in batches:
        g = model.forward(utts(idx), lid=[LIDS[i] for i in idx], textnorm=[TEXTNORMS[i] for i in idx])
        want.append((greedy_tokens(g), model.align(greedy_tokens(g))))
    model.set_inflight(2)
    try:
        model.warm_up(2, 16000)
        gate = threading.Barrier(2)
        res, errs = [None, None], []

        def work(k):
            try:
                idx = batches[k][0]
                g = model.forward(utts(idx), lid=[LIDS[i] for i in idx], textnorm=[TEXTNORMS[i] for i in idx])
                gate.wait(timeout=60)                                # both forwards are done before either aligns
                res[k] = (greedy_tokens(g), model.align(greedy_tokens(g)))
            except Exception as e:                                   # noqa: BLE001
                errs.append(e)
                gate.abort()

        th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for k in range(2):
            assert res[k][0] == want[k][0]
            for key in ("begin", "end"):
                assert [x.tolist() for x in res[k][1][key]] == [x.tolist() for x in want[k][1][key]]
            assert res[k][1]["score"].tobytes() == want[k][1]["score"].tobytes()
    finally:
        model.set_inflight(1)
