"""CPU: token spans from the fire frames of the CIF scan (csrc/host/timestamp.cpp CifTimestamps, through pfhip_cif_timestamps).

The rule is an extension (the reference stamps only through its timestamp head) and is stated in include/pfhip.h; `rule` below is
its restatement.  Frames are small integers and 60 ms a row, so begin / end are compared as float32 of the same double expression.
"""
import numpy as np
import pytest

F32 = np.float32
PFHIP_ERR_ARG, PFHIP_ERR_CAPACITY = 1, 5


@pytest.fixture(scope="module")
def ts(pkg):
    import os
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    pkg.load_lib()
    return pkg.cif_timestamps


def rule(fire_frame, n_chars, n_frames, frame_ms=60.0, begin_ms=0.0):
    """MAX_TOKEN_DURATION = 30 x 20 ms and START_END_THRESHOLD = 5 x 20 ms of TimestampOnnx (util.cpp:838-963), as times."""
    if n_chars <= 0:
        return []
    maxtok = 600.0 / frame_ms
    sec = lambda f: float(F32(f * frame_ms / 1000.0 + begin_ms / 1000.0))
    spans, prev = [], 0.0
    for k in range(n_chars):
        e = min(float(fire_frame[k]) + 1.0, float(n_frames))
        b = max(prev, e - maxtok)
        if b > prev:
            spans.append((sec(prev), sec(b), True))
        spans.append((sec(b), sec(e), False))
        prev = e
    if (n_frames - prev) * frame_ms > 100.0:
        spans.append((sec(prev), sec(n_frames), True))
    else:
        spans[-1] = (spans[-1][0], sec(n_frames), False)
    return spans


def approx(spans):
    return [(round(b, 6), round(e, 6), s) for b, e, s in spans]


def test_known_answer(ts):
    """The header's example: 40 rows of 60 ms, fires in rows 4, 9, 30, 33 and the tail slot's "</s>" (40), four characters."""
    got = ts([4, 9, 30, 33, 40], 4, 40, 60.0)
    want = [(0.00, 0.30, False), (0.30, 0.60, False), (0.60, 1.26, True), (1.26, 1.86, False), (1.86, 2.04, False), (2.04, 2.40, True)]
    assert [s for _, _, s in got] == [s for _, _, s in want]
    assert np.allclose([(b, e) for b, e, _ in got], [(b, e) for b, e, _ in want], rtol=0, atol=1e-6)
    assert got == rule([4, 9, 30, 33, 40], 4, 40)


def test_gap_of_maxtok_frames_has_no_sil_and_one_more_has(ts):
    # maxtok = 600 / 60 = 10 rows.  Token 0 ends with row 4 (e = 5); a fire in row 14 ends at 15: the gap is exactly 10 rows
    got = ts([4, 14], 2, 15, 60.0)
    assert [s for _, _, s in got] == [False, False]
    assert approx(got) == [(0.0, 0.3, False), (0.3, 0.9, False)]
    # a fire in row 15 ends at 16: 11 rows, of which the first is <sil>
    got = ts([4, 15], 2, 16, 60.0)
    assert approx(got) == [(0.0, 0.3, False), (0.3, 0.36, True), (0.36, 0.96, False)]


def test_trailing_gap_absorbed_or_sil(ts):
    # one row (60 ms <= START_END_THRESHOLD) after the last token: absorbed into it
    assert approx(ts([4, 8], 2, 10, 60.0)) == [(0.0, 0.3, False), (0.3, 0.6, False)]
    # two rows (120 ms): a <sil> span
    assert approx(ts([4, 8], 2, 11, 60.0)) == [(0.0, 0.3, False), (0.3, 0.54, False), (0.54, 0.66, True)]


def test_two_fires_in_one_row_give_a_zero_length_token(ts):
    got = ts([3, 3, 6], 3, 7, 60.0)
    assert approx(got) == [(0.0, 0.24, False), (0.24, 0.24, False), (0.24, 0.42, False)]


def test_begin_time_offset(ts):
    base = ts([4, 9, 30, 33, 40], 4, 40, 60.0)
    moved = ts([4, 9, 30, 33, 40], 4, 40, 60.0, begin_time=1500.0)
    assert [s for _, _, s in moved] == [s for _, _, s in base]
    assert np.allclose([(b, e) for b, e, _ in moved], [(b + 1.5, e + 1.5) for b, e, _ in base], rtol=0, atol=1e-6)
    assert moved == rule([4, 9, 30, 33, 40], 4, 40, 60.0, 1500.0)


def test_no_characters_no_spans(ts):
    assert ts([4, 9], 0, 40, 60.0) == []
    assert ts([], 0, 0, 60.0) == []


def test_bad_arguments(ts, pkg):
    for args in (([4, 9], 3, 40, 60.0),          # more characters than fires
                 ([4, 9], -1, 40, 60.0), ([4, 9], 2, -1, 60.0), ([4, 9], 2, 40, 0.0), ([4, 9], 2, 40, -60.0)):
        with pytest.raises(pkg.PfhipError) as e:
            ts(*args)
        assert e.value.status == PFHIP_ERR_ARG, args
    with pytest.raises(pkg.PfhipError) as e:
        ts([4, 9], 2, 40, 60.0, begin_time=-1.0)
    assert e.value.status == PFHIP_ERR_ARG


def test_capacity_error_carries_the_count(ts, pkg):
    with pytest.raises(pkg.PfhipError) as e:
        ts([4, 9, 30, 33, 40], 4, 40, 60.0, cap=5)
    assert e.value.status == PFHIP_ERR_CAPACITY and e.value.needed == 6
    assert len(ts([4, 9, 30, 33, 40], 4, 40, 60.0, cap=6)) == 6


def test_agrees_with_the_restatement_on_random_fire_lists(ts):
    rng = np.random.default_rng(606)
    sil = zero = absorbed = 0
    for _ in range(200):
        T = int(rng.integers(1, 120))
        n = int(rng.integers(1, 40))
        fires = np.sort(rng.integers(0, T + 1, n)).astype(np.int32)        # non-decreasing, T = the tail slot
        n_chars = int(rng.integers(0, n + 1))
        frame_ms = float(rng.choice([60.0, 30.0, 20.0]))
        begin = float(rng.integers(0, 5000))
        got, want = ts(fires, n_chars, T, frame_ms, begin_time=begin), rule(fires, n_chars, T, frame_ms, begin)
        assert got == want, (list(fires), n_chars, T, frame_ms, begin)
        toks = [(b, e) for b, e, s in got if not s]
        assert len(toks) == n_chars
        assert all(b <= e for b, e, _ in got) and all(got[i][1] == got[i + 1][0] for i in range(len(got) - 1))      # ordered, gapless
        if got:
            assert got[0][0] == float(F32(begin / 1000.0)) and got[-1][1] == float(F32(T * frame_ms / 1000.0 + begin / 1000.0))
        sil += sum(1 for _, _, s in got if s)
        zero += sum(1 for b, e in toks if b == e)
        absorbed += int(bool(got) and not got[-1][2])
    assert sil > 50 and zero > 50 and absorbed > 20        # the list exercised every branch
