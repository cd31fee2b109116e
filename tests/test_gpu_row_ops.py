"""GPU: the scan, cache and row kernels that only whole-model tests reached, each through its own operator entry
(include/pfhip_ops.h) against a plain reference of the same operation.

Where a kernel does the same fp32 operations in the same order as the oracle's scalar restatement (the library is built with
-ffp-contract=off) the comparison is np.array_equal.  Everywhere else the reference is fp64 and the bound is derived: a sum of n fp32
terms in any order errs by at most n * 2^-24 * sum(|terms|), computed per element from the fp64 terms, with the n each test states.
Every output element of every case is compared; every test prints its largest error over bound before it asserts.
"""
import importlib

import numpy as np
import pytest

from oracle import paraformer as P
from oracle import paraformer_online as PO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32, F64 = np.float32, np.float64
U = 2.0 ** -24           # fp32 unit roundoff
CANARY = F32(-1234.5)


@pytest.fixture(scope="module")
def ops(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    return importlib.import_module("asr_2pass_amd.ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def report(name, err, bound):
    """Largest error over bound (elements whose bound is 0 must have no error); printed, returned for the assertion."""
    err, bound = np.asarray(err, F64), np.asarray(bound, F64)
    assert np.all(err[bound == 0] == 0), f"{name}: an error where the bound is zero"
    ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0
    print(f"{name}: max err / bound = {ratio:.3f} (max abs err {float(err.max()) if err.size else 0.0:.3e})")
    return ratio


# ---- cif_stream ---------------------------------------------------------------------------------------------------------------
THR, TAIL = F32(1.0), F32(0.45)


def oracle_stream(D, pre, suf):
    """A ParaformerOnline holding only the state CifSearch reads: the method itself is what runs."""
    o = PO.ParaformerOnline.__new__(PO.ParaformerOnline)
    o.chunk_size = [pre, suf - pre, 0]
    o.encoder_size = D
    o.cif_threshold, o.tail_alphas = THR, TAIL
    o.is_last_chunk = False
    return o


def sixteenths(rng, n):
    """Multiples of 1/16 in [0, 1]: alpha + integrate is exact in fp32 and meets the threshold exactly, often."""
    return (rng.integers(0, 17, n) / 16.0).astype(F32)


# (n, pre, suf, is_last) of the six connections of one launch
CIF_CONNS = [(20, 5, 15, 0), (20, 0, 20, 0), (1, 0, 20, 0), (0, 5, 15, 1), (13, 5, 15, 1), (20, 5, 15, 0)]


def run_cif_chunk(ops, oracles, conns, enc, alphas, carry, emb_rows, D):
    """One launch for all connections and one CifSearch call per oracle; returns (emb, n_fire, oracle fires per connection)."""
    B = len(conns)
    row_off = np.concatenate([[0], np.cumsum([c[0] for c in conns])[:-1]]).astype(np.int32)
    emb = torch.full((B, emb_rows, D), float(CANARY), dtype=torch.float32, device="cuda")
    n_fire = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ops.cif_stream(dev(enc), dev(alphas), row_off, [c[0] for c in conns], [c[3] for c in conns], [c[1] for c in conns],
                   [c[2] for c in conns], carry, D, THR, TAIL, emb, n_fire)
    fires = []
    for b, (n, pre, suf, is_last) in enumerate(conns):
        o = oracles[b]
        o.chunk_size = [pre, suf - pre, 0]
        o.is_last_chunk = bool(is_last)
        r = row_off[b]
        fires.append(o.CifSearch([enc[r + i] for i in range(n)], alphas[r:r + n]))
    return host(emb), host(n_fire), fires


@pytest.mark.parametrize("D", [320, 512, 516])       # 516: cif_stream_kernel<2> with four channels in its second slot
def test_cif_stream_chained_bit_exact(ops, D):
    """Four chunks of six connections chained through the carry buffer == four CifSearch calls on one oracle state each: emitted
    rows, n_fire, carry hidden row and carry alpha after every chunk, bit for bit.  Carry buffers sit back to back (D + 1 floats
    each), so a write past a connection's D + 1 floats lands in its neighbour's carry."""
    rng = np.random.default_rng(1000 + D)
    B, emb_rows = len(CIF_CONNS), 24
    carry0 = np.zeros((B, D + 1), F32)
    carry0[:, :D] = rng.standard_normal((B, D))
    carry0[:, D] = rng.integers(1, 16, B) / 16.0
    carry0[5, D] = 0.0                                   # a carry that comes in with integrate = 0 and a hidden row that is not zero
    oracles = []
    for b in range(B):
        o = oracle_stream(D, 5, 15)
        o.hidden_cache_, o.alphas_cache_ = [carry0[b, :D].copy()], [F32(carry0[b, D])]
        oracles.append(o)
    carry = dev(carry0)
    exact_hits = 0
    for k in range(4):
        conns = [CIF_CONNS[(b + k) % B] for b in range(B)]          # every connection meets every window shape
        M = sum(c[0] for c in conns)
        enc = rng.standard_normal((M, D)).astype(F32)
        alphas = sixteenths(rng, M)
        before = [F32(o.alphas_cache_[0]) for o in oracles]
        emb, n_fire, fires = run_cif_chunk(ops, oracles, conns, enc, alphas, carry, emb_rows, D)
        got_carry = host(carry)
        for b in range(B):
            assert n_fire[b] == len(fires[b]), (k, b, n_fire[b], len(fires[b]))
            want = np.stack(fires[b]) if fires[b] else np.zeros((0, D), F32)
            assert np.array_equal(emb[b, :len(fires[b])], want), (k, b)
            assert np.all(emb[b, len(fires[b]):] == CANARY), (k, b)
            assert np.array_equal(got_carry[b, :D], oracles[b].hidden_cache_[0]), (k, b)
            assert got_carry[b, D] == oracles[b].alphas_cache_[0], (k, b)
        # how often this chunk met the threshold exactly (what random alphas never do): counted on the oracle's own recurrence
        row = 0
        for b, (n, pre, suf, is_last) in enumerate(conns):
            integ = before[b]
            a = alphas[row:row + n].copy()
            a[:pre] = 0
            a[suf:] = 0
            for x in list(a) + ([TAIL] if is_last else []):
                s = F32(F32(x) + integ)
                exact_hits += int(s == THR)
                integ = s if s < THR else F32(s - THR)
            row += n
    print(f"cif_stream D={D}: alpha + integrate == threshold met {exact_hits} times")
    assert exact_hits >= 4


def test_cif_stream_overflow_keeps_neighbours(ops):
    """emb_rows = 4 and a connection that fires 6 times: n_fire says 6, rows 0..3 are right, and the neighbours' emb blocks hold
    nothing but their own fires."""
    D, emb_rows = 512, 4
    rng = np.random.default_rng(77)
    conns = [(20, 5, 15, 0), (20, 5, 15, 0), (20, 5, 15, 0)]
    enc = rng.standard_normal((60, D)).astype(F32)
    alphas = np.zeros(60, F32)
    alphas[5:8] = [0.5, 0.25, 0.5]                       # connection 0: one fire
    alphas[20 + 6:20 + 12] = 1.0                         # connection 1: six fires, one per frame
    alphas[40 + 14] = 1.0                                # connection 2: one fire on the last counted frame
    carry0 = np.zeros((3, D + 1), F32)
    carry0[:, :D] = rng.standard_normal((3, D))
    carry0[:, D] = [0.25, 0.0, 0.5]
    oracles = []
    for b in range(3):
        o = oracle_stream(D, 5, 15)
        o.hidden_cache_, o.alphas_cache_ = [carry0[b, :D].copy()], [F32(carry0[b, D])]
        oracles.append(o)
    carry = dev(carry0)
    emb, n_fire, fires = run_cif_chunk(ops, oracles, conns, enc, alphas, carry, emb_rows, D)
    assert [len(f) for f in fires] == [1, 6, 1]
    assert list(n_fire) == [1, 6, 1]
    assert np.array_equal(emb[1], np.stack(fires[1][:4]))
    for b in (0, 2):
        assert np.array_equal(emb[b, 0], fires[b][0])
        assert np.all(emb[b, 1:] == CANARY)
    got_carry = host(carry)
    for b in range(3):
        assert np.array_equal(got_carry[b, :D], oracles[b].hidden_cache_[0])
        assert got_carry[b, D] == oracles[b].alphas_cache_[0]


def test_cif_stream_refuses_what_the_kernel_assumes(ops, pkg):
    z = torch.zeros((4, 2048), dtype=torch.float32, device="cuda")
    nf = torch.zeros(1, dtype=torch.int32, device="cuda")
    emb = torch.zeros((1, 4, 1028), dtype=torch.float32, device="cuda")
    with pytest.raises(pkg.PfhipError):                 # D > 1024: a third channel slot the kernel does not have
        ops.cif_stream(z, z[0], [0], [1], [0], [0], [1], z, 1028, THR, TAIL, emb, nf)
    with pytest.raises(pkg.PfhipError):                 # a NULL buffer
        ops.cif_stream(z, None, [0], [1], [0], [0], [1], z, 512, THR, TAIL, emb, nf)


# ---- fsmn_cached --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer", [0, 2])
@pytest.mark.parametrize("C", [320, 512])
def test_fsmn_cached(ops, C, layer):
    """out (aliasing res, as stream.cpp calls it) against fp64 with n = 13 (11 taps and two adds); the layer's new cache is a copy:
    array_equal to the last 10 rows of [cache; t2]; the n_tok = 0 connection's cache and every other layer's cache are bit-identical
    before and after.  Largest error over bound measured on the MI355X: 0.244."""
    rng = np.random.default_rng(C + layer)
    n_tok = [0, 1, 9, 10, 11, 37]
    B, layers = len(n_tok), 4
    tok_off = np.concatenate([[0], np.cumsum(n_tok)[:-1]]).astype(np.int32)
    M = sum(n_tok)
    t2 = rng.standard_normal((M, C)).astype(F32)
    res = rng.standard_normal((M, C)).astype(F32)
    w = (rng.standard_normal((C, 11)) * 0.3).astype(F32)
    cache0 = rng.standard_normal((B, layers, 10, C)).astype(F32)
    d_res, d_cache = dev(res), dev(cache0)
    ops.fsmn_cached(dev(t2), dev(w), d_res, d_res, tok_off, n_tok, d_cache, layer)
    out, cache1 = host(d_res), host(d_cache)
    err, bound = [], []
    for b, (o, n) in enumerate(zip(tok_off, n_tok)):
        other = [l for l in range(layers) if l != layer]
        assert np.array_equal(cache1[b, other], cache0[b, other]), b
        if n == 0:
            assert np.array_equal(cache1[b], cache0[b])
            continue
        xcat = np.concatenate([cache0[b, layer], t2[o:o + n]])
        assert np.array_equal(cache1[b, layer], xcat[-10:]), b
        terms = np.stack([xcat[j:j + n].astype(F64) * w[:, j].astype(F64)[None, :] for j in range(11)]
                         + [t2[o:o + n].astype(F64), res[o:o + n].astype(F64)])
        err.append(np.abs(out[o:o + n] - terms.sum(0)))
        bound.append(13 * U * np.abs(terms).sum(0))
    assert report(f"fsmn_cached C={C} layer={layer}", np.concatenate(err), np.concatenate(bound)) <= 1.0


def test_fsmn_cached_refuses_what_the_kernel_assumes(ops, pkg):
    x = torch.zeros((4, 322), dtype=torch.float32, device="cuda")
    w = torch.zeros((322, 11), dtype=torch.float32, device="cuda")
    cache = torch.zeros((1, 1, 10, 322), dtype=torch.float32, device="cuda")
    with pytest.raises(pkg.PfhipError):                 # C % 4: the kernel moves four channels per 16-byte access
        ops.fsmn_cached(x, w, x, x, [0], [4], cache, 0)
    with pytest.raises(pkg.PfhipError):
        ops.fsmn_cached(x[:, :320], w, None, x, [0], [4], cache, 0)


# ---- fsmn_causal20 ------------------------------------------------------------------------------------------------------------
VAD_C, VAD_LAYERS, VAD_LAYER = 128, 3, 1


def causal20_launch(ops, p, ld, w, row_off, T, final, cache_in):
    """One launch on rows of p (given [rows, C], staged with row stride ld and canary pads): (out [rows, C], cache_out, pads ok)."""
    B = len(T)
    rows = p.shape[0]
    pp = np.full((rows, ld), CANARY, F32)
    pp[:, :VAD_C] = p
    d_out = torch.full((rows, ld), float(CANARY), dtype=torch.float32, device="cuda")
    d_cin = dev(cache_in)
    d_cout = torch.full((B, VAD_LAYERS, 19, VAD_C), float(CANARY), dtype=torch.float32, device="cuda")
    ops.fsmn_causal20(dev(pp), dev(w), row_off, T, final, d_cin, d_cout, VAD_LAYER, VAD_C, d_out)
    assert np.array_equal(host(d_cin), cache_in)                    # the input caches are never written
    out = host(d_out)
    assert np.all(out[:, VAD_C:] == CANARY)
    return out[:, :VAD_C], host(d_cout)


def causal20_check(name, p, w, row_off, T, final, cache_in, out, cache_out):
    """fp64 with n = 21 (20 taps and one add); cache_out array_equal to the last 19 rows of [cache_in; p], untouched where final.
    Largest error over bound measured on the MI355X: 0.170."""
    err, bound = [], []
    covered = np.zeros(p.shape[0], bool)
    for b, (o, n) in enumerate(zip(row_off, T)):
        xcat = np.concatenate([cache_in[b, VAD_LAYER], p[o:o + n]])
        terms = np.stack([xcat[j:j + n].astype(F64) * w[:, j].astype(F64)[None, :] for j in range(20)] + [p[o:o + n].astype(F64)])
        err.append(np.abs(out[o:o + n] - terms.sum(0)))
        bound.append(21 * U * np.abs(terms).sum(0))
        covered[o:o + n] = True
        other = [l for l in range(VAD_LAYERS) if l != VAD_LAYER]
        assert np.all(cache_out[b, other] == CANARY), b
        if final[b]:
            assert np.all(cache_out[b] == CANARY), b
        else:
            assert np.array_equal(cache_out[b, VAD_LAYER], xcat[-19:]), (b, n)      # T < 19: old cache rows survive
    assert np.all(out[~covered] == CANARY)                                          # rows between the connections' windows
    return report(name, np.concatenate(err), np.concatenate(bound))


@pytest.mark.parametrize("ld", [128, 136])
def test_fsmn_causal20(ops, ld):
    rng = np.random.default_rng(ld)
    w = (rng.standard_normal((VAD_C, 20)) * 0.2).astype(F32)
    # four connections at different row offsets (with unused rows between them), the last one on its final call
    T, row_off, final = [1, 18, 33, 70], [2, 5, 26, 61], [0, 0, 0, 1]
    p = rng.standard_normal((140, VAD_C)).astype(F32)
    cache_in = rng.standard_normal((4, VAD_LAYERS, 19, VAD_C)).astype(F32)
    out, cache_out = causal20_launch(ops, p, ld, w, row_off, T, final, cache_in)
    worst = causal20_check(f"fsmn_causal20 ld={ld} packed", p, w, row_off, T, final, cache_in, out, cache_out)
    for t in (19, 20, 31, 32):                           # the cache length and the kernel's 32-row time tile, either side
        p1 = rng.standard_normal((t, VAD_C)).astype(F32)
        c1 = rng.standard_normal((1, VAD_LAYERS, 19, VAD_C)).astype(F32)
        for fin in (0, 1):
            o1, co1 = causal20_launch(ops, p1, ld, w, [0], [t], [fin], c1)
            worst = max(worst, causal20_check(f"fsmn_causal20 ld={ld} T={t} final={fin}", p1, w, [0], [t], [fin], c1, o1, co1))
    assert worst <= 1.0


@pytest.mark.parametrize("ld", [128, 136])
def test_fsmn_causal20_split_equals_one_pass(ops, ld):
    """A 70-row input split at T1 and chained through the cache == the one-pass output bit for bit: a row's taps and their order do
    not depend on whether the window came from the cache or from p."""
    rng = np.random.default_rng(7 + ld)
    w = (rng.standard_normal((VAD_C, 20)) * 0.2).astype(F32)
    p = rng.standard_normal((70, VAD_C)).astype(F32)
    c0 = rng.standard_normal((1, VAD_LAYERS, 19, VAD_C)).astype(F32)
    whole, c_whole = causal20_launch(ops, p, ld, w, [0], [70], [0], c0)
    for t1 in (1, 18, 19, 20, 32, 33):
        a, ca = causal20_launch(ops, p[:t1], ld, w, [0], [t1], [0], c0)
        c1 = c0.copy()
        c1[0, VAD_LAYER] = ca[0, VAD_LAYER]
        b, cb = causal20_launch(ops, p[t1:], ld, w, [0], [70 - t1], [0], c1)
        assert np.array_equal(np.concatenate([a, b]), whole), t1
        assert np.array_equal(cb[0, VAD_LAYER], c_whole[0, VAD_LAYER]), t1


def test_fsmn_causal20_refuses_what_the_kernel_assumes(ops, pkg):
    def z(*shape):
        return torch.zeros(shape, dtype=torch.float32, device="cuda")
    w, cin, cout = z(128, 20), z(1, 1, 19, 128), z(1, 1, 19, 128)
    with pytest.raises(pkg.PfhipError):                 # ld % 4
        ops.fsmn_causal20(z(4, 130), w, [0], [4], [0], cin, cout, 0, 128, z(4, 128))
    with pytest.raises(pkg.PfhipError):                 # C % 4
        ops.fsmn_causal20(z(4, 128), w, [0], [4], [0], cin, cout, 0, 126, z(4, 128))
    with pytest.raises(pkg.PfhipError):                 # cache_out must not be cache_in
        ops.fsmn_causal20(z(4, 128), w, [0], [4], [0], cin, cin, 0, 128, z(4, 128))
    with pytest.raises(pkg.PfhipError):
        ops.fsmn_causal20(z(4, 128), w, [0], [4], [0], cin, None, 0, 128, z(4, 128))


# ---- softmax_rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 248])
@pytest.mark.parametrize("M", [1, 4, 5])
def test_softmax_rows(ops, M, N):
    """Per element against fp64: (|x - m| + N / 64 + 16) * 2^-23 * y_ref — |x - m| for the rounded subtraction in the exponent,
    N / 64 for the sum, 16 for expf, the shuffle tree and the divide; absolute 1e-37 where y_ref is below 1e-37.  Row kinds rotate
    (all equal / spanning -80 .. +80 / within +-10) so that every M sees every kind in every row position.
    Largest error over bound measured on the MI355X: 0.372."""
    rng = np.random.default_rng(M * 1000 + N)
    ldx = 256
    worst = 0.0
    for shift in range(3):
        x = np.full((M, ldx), 100.0, F32)                # pad columns hold +100 and must be ignored
        for r in range(M):
            kind = (r + shift) % 3
            if kind == 0:
                x[r, :N] = F32(rng.uniform(-10, 10))
            elif kind == 1:
                x[r, :N] = rng.permutation(np.linspace(-80.0, 80.0, N)).astype(F32) if N > 1 else F32(-80.0)
            else:
                x[r, :N] = rng.uniform(-10, 10, N).astype(F32)
        y = torch.full((M + 3, N), float(CANARY), dtype=torch.float32, device="cuda")
        col0 = torch.full((M + 3,), float(CANARY), dtype=torch.float32, device="cuda")
        ops.softmax_rows(dev(x), M, N, y, col0)
        y, col0 = host(y), host(col0)
        assert np.all(y[M:] == CANARY) and np.all(col0[M:] == CANARY)
        assert np.array_equal(col0[:M], y[:M, 0])
        xd = x[:, :N].astype(F64)
        m = xd.max(1, keepdims=True)
        e = np.exp(xd - m)
        ref = e / e.sum(1, keepdims=True)
        err = np.abs(y[:M] - ref)
        bound = (np.abs(xd - m) + N / 64.0 + 16.0) * 2.0 ** -23 * ref
        tiny = ref < 1e-37
        assert np.all(err[tiny] <= 1e-37)
        if np.any(~tiny):
            worst = max(worst, report(f"softmax_rows M={M} N={N} shift={shift}", err[~tiny], bound[~tiny]))
    assert worst <= 1.0


# ---- im2col3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [320, 512])
def test_im2col3_is_a_gather(ops, D):
    """Utterances of 1, 2 and 7 rows packed back to back, every value nonzero, one more nonzero row on either side of the pack: a
    wrong edge reads a neighbour's row instead of zero.  array_equal with numpy."""
    rng = np.random.default_rng(D)
    lens = [1, 2, 7]
    M = sum(lens)
    ldh, ldc = D + 4, 3 * D + 4
    hbuf = (rng.uniform(1.0, 2.0, (M + 2, ldh)) * rng.choice([-1.0, 1.0], (M + 2, ldh))).astype(F32)
    d_hbuf = dev(hbuf)
    row_pos = np.concatenate([np.arange(n) for n in lens]).astype(np.int32)
    row_len = np.concatenate([np.full(n, n) for n in lens]).astype(np.int32)
    col = torch.full((M, ldc), float(CANARY), dtype=torch.float32, device="cuda")
    ops.im2col3(d_hbuf[1:], dev(row_pos), dev(row_len), D, out=col)
    got = host(col)
    h = hbuf[1:1 + M, :D]
    want = np.zeros((M, 3 * D), F32)
    for row in range(M):
        for j in range(3):
            tt = row_pos[row] + j - 1
            if 0 <= tt < row_len[row]:
                want[row, j * D:(j + 1) * D] = h[row + j - 1]
    assert np.array_equal(got[:, :3 * D], want)
    assert np.all(got[:, 3 * D:] == CANARY)


def test_im2col3_refuses_what_the_kernel_assumes(ops, pkg):
    h = torch.zeros((4, 322), dtype=torch.float32, device="cuda")
    i4 = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(pkg.PfhipError):                 # ld % 4
        ops.im2col3(h, i4, i4, 320)
    with pytest.raises(pkg.PfhipError):                 # D % 4
        ops.im2col3(h[:, :320].contiguous(), i4, i4, 318)


# ---- alpha, alpha2 ------------------------------------------------------------------------------------------------------------
def alpha_case(rng, M, D, ld):
    """Rows of mixed scale; row 0 (and row 4 where there is one) driven far below the noise threshold, row 1 above it."""
    w = (rng.standard_normal(D) / np.sqrt(D)).astype(F32)
    o = np.full((M, ld), 1e6, F32)                       # pad columns: huge, and never read
    o[:, :D] = rng.standard_normal((M, D)) * rng.uniform(0.5, 3.0, (M, 1))
    for r in (0, 4):
        if r < M:
            o[r, :D] = -np.sign(w) * rng.uniform(0.5, 1.5, D)         # logit about -sum |w| ~ -0.8 sqrt(D): sigmoid < 1e-6
    if M > 1:
        o[1, :D] = np.sign(w) * rng.uniform(0.0, 0.2, D)              # and one row safely above it
    return o, w


def alpha_reference(o, w, b, smooth, noise, D):
    """fp64 alpha and its absolute bound smooth * (0.25 * logit_bound + 8 * 2^-24), logit_bound = n * 2^-24 * sum |terms| with
    n = D / 64 + 70: at most D / 256 accumulation steps of 4 terms per lane, then 64 lanes, the bias and slack for the order.
    Largest error over bound measured on the MI355X: alpha 0.033, alpha2 0.013."""
    terms = o[:, :D].astype(F64) * w.astype(F64)[None, :]
    logit = terms.sum(1) + F64(b)
    n = D / 64 + 70
    logit_bound = n * U * (np.abs(terms).sum(1) + abs(F64(b)))
    ref = np.maximum(1.0 / (1.0 + np.exp(-logit)) * F64(smooth) - F64(noise), 0.0)
    return ref, F64(smooth) * (0.25 * logit_bound + 8 * U), logit


@pytest.mark.parametrize("M", [1, 4, 5, 9])
@pytest.mark.parametrize("D", [320, 512])
def test_alpha(ops, D, M):
    rng = np.random.default_rng(D * 10 + M)
    o, w = alpha_case(rng, M, D, D + 8)
    b, smooth, noise = F32(-0.3), F32(1.0), F32(0.45)
    got = host(ops.alpha(dev(o), dev(w), dev(np.asarray([b], F32)), smooth, noise, M, D))
    ref, bound, logit = alpha_reference(o, w, b, smooth, noise, D)
    assert logit[0] < -8 and got[0] == 0.0              # below the noise threshold: exactly 0
    assert M == 1 or (ref[1] > 0.1 and got[1] > 0.1)
    assert report(f"alpha D={D} M={M}", np.abs(got - ref), bound) <= 1.0


@pytest.mark.parametrize("M", [1, 4, 5, 9])
def test_alpha2(ops, M):
    D = 1024
    rng = np.random.default_rng(M)
    o, w = alpha_case(rng, M, D, D)
    b, smooth, noise = F32(0.2), F32(0.25), F32(0.01)
    got = host(ops.alpha2(dev(o), dev(w), b, smooth, noise, M, D))
    ref, bound, logit = alpha_reference(o, w, b, smooth, noise, D)      # n = D / 64 + 70 as for alpha: D / 256 steps of 4 terms one by one
    assert logit[0] < -8 and got[0] == 0.0
    assert M == 1 or (ref[1] > 0.1 and got[1] > 0.1)
    assert report(f"alpha2 M={M}", np.abs(got - ref), bound) <= 1.0


def test_alpha_refuses_what_the_kernel_assumes(ops, pkg):
    o = torch.zeros((4, 322), dtype=torch.float32, device="cuda")
    w = torch.zeros(320, dtype=torch.float32, device="cuda")
    with pytest.raises(pkg.PfhipError):                 # ld % 4
        ops.alpha(o, w, w, 1.0, 0.0, 4, 320)
    with pytest.raises(pkg.PfhipError):                 # D % 4
        ops.alpha2(o[:, :320].contiguous(), w, 0.0, 1.0, 0.0, 4, 318)


# ---- us_cif -------------------------------------------------------------------------------------------------------------------
US_THR = F32(F32(1.0) - F32(1e-4))                       # what the forward passes: cif_threshold - 1e-4f


def us_cif_check(ops, name, a2, lens, toks, thr):
    """us_alphas against fp64 with relative bound (L + 4) * 2^-24; us_peaks bit for bit cif_wo_hidden fed the kernel's own
    us_alphas and the same float threshold (the scan is serial fp32 additions: nothing is reordered, and a decision at the
    threshold cannot fail the test through the alphas' rounding).  Largest error over bound measured on the MI355X: 0.016."""
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    us_alphas, us_peaks = ops.us_cif(dev(a2), dev(off), dev(np.asarray(lens, np.int32)), dev(np.asarray(toks, np.int32)), thr)
    us_alphas, us_peaks = host(us_alphas), host(us_peaks)
    worst, fires = 0.0, 0
    for o, L, tok in zip(off, lens, toks):
        x = a2[o:o + L].astype(F64)
        ref = x * (F64(tok) / x.sum())
        worst = max(worst, report(f"{name} L={L} tok={tok}", np.abs(us_alphas[o:o + L] - ref), (L + 4) * U * ref))
        want = P.cif_wo_hidden(us_alphas[o:o + L], thr)
        assert np.array_equal(us_peaks[o:o + L], want), (L, tok)
        fires += int(np.sum(want >= thr))
    return worst, fires


def test_us_cif(ops):
    rng = np.random.default_rng(5)
    lens, toks = [1, 255, 256, 257, 1500, 4500], [1, 17, 400, 1, 17, 400]
    a2 = np.maximum(rng.uniform(-0.05, 0.24, sum(lens)), 0.0).astype(F32)      # relu output: some exact zeros
    a2[0] = F32(0.125)
    worst, fires = us_cif_check(ops, "us_cif", a2, lens, toks, US_THR)
    assert fires >= 600
    assert worst <= 1.0


def test_us_cif_meets_the_threshold_exactly(ops):
    """Alphas in sixteenths that sum to token_num exactly: the rescale is by 1.0, every running sum is exact and the scan meets its
    threshold (1.0 here) exactly, which alphas from a sigmoid never do — the '>=' of the fire test decides."""
    rng = np.random.default_rng(6)
    lens, a2, toks = [255, 256, 257], [], []
    for L in lens:
        a = (rng.integers(0, 5, L) / 16.0).astype(F32)
        a[-1] = 0
        a[-1] = F32(np.ceil(a.sum()) - a.sum())
        a2.append(a)
        toks.append(int(round(float(a.sum()))))
    a2 = np.concatenate(a2)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    worst, _ = us_cif_check(ops, "us_cif exact", a2, lens, toks, F32(1.0))
    assert worst == 0.0                                  # the rescale by exactly 1.0 changes nothing
    exact = sum(int(np.sum(P.cif_wo_hidden(a2[o:o + L], F32(1.0)) == F32(1.0))) for o, L in zip(off, lens))
    print(f"us_cif exact: the scan met its threshold exactly {exact} times")
    assert exact >= 10


def test_us_cif_16500_frames(ops):
    """One utterance of 16500 upsampled frames (5500 encoder frames, 330 s): 66000 bytes of dynamic LDS on top of 1 KB static, past
    64 KB.  The entry must return 0 (the wrapper raises otherwise) and both outputs pass the same checks.  On the MI355X the runtime
    takes the launch as it is (error over bound 0.0005)."""
    rng = np.random.default_rng(8)
    a2 = np.maximum(rng.uniform(-0.05, 0.24, 16500), 0.0).astype(F32)
    worst, fires = us_cif_check(ops, "us_cif long", a2, [16500], [400], US_THR)
    assert fires >= 395
    assert worst <= 1.0


# ---- lstm_cell ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 3, 40])
def test_lstm_cell(ops, H):
    """Three steps, D = 512.  c and h of every step against an fp64 step from the c that went in, absolute bound
    16 * 2^-24 * (1 + |c_prev|); sel rows equal h bit for bit at t == len - 1 and keep their canary at every other t.
    Largest error over bound measured on the MI355X: 0.145."""
    D = 512
    rng = np.random.default_rng(H)
    lens = (np.arange(H) % 3 + 1).astype(np.int32)
    if H == 1:
        lens[:] = 2
    c = dev((rng.standard_normal((H, D)) * 2).astype(F32))
    h = torch.full((H, D), float(CANARY), dtype=torch.float32, device="cuda")
    sel = torch.full((H, D), float(CANARY), dtype=torch.float32, device="cuda")
    want_sel = np.full((H, D), CANARY, F32)
    d_lens = dev(lens)
    worst = 0.0

    def sig(v):
        return 1.0 / (1.0 + np.exp(-v))
    for t in range(3):
        G = (rng.standard_normal((H, 4 * D)) * 3).astype(F32)
        c_prev = host(c).astype(F64)
        ops.lstm_cell(dev(G), c, h, d_lens, t, sel)
        g = G.astype(F64)
        c_ref = sig(g[:, D:2 * D]) * c_prev + sig(g[:, :D]) * np.tanh(g[:, 2 * D:3 * D])
        h_ref = sig(g[:, 3 * D:]) * np.tanh(c_ref)
        bound = 16 * U * (1 + np.abs(c_prev))
        got_c, got_h = host(c), host(h)
        worst = max(worst, report(f"lstm_cell H={H} t={t} c", np.abs(got_c - c_ref), bound),
                    report(f"lstm_cell H={H} t={t} h", np.abs(got_h - h_ref), bound))
        want_sel[lens - 1 == t] = got_h[lens - 1 == t]
        assert np.array_equal(host(sel), want_sel), t
    assert worst <= 1.0
