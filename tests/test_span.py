"""The span search without a GPU: the checker's three statements of the definition (tests/span_ref.py) agree, the
word-snapping rule, the argument errors of the Python and C interfaces, and one pin on what the definition is FOR."""
import numpy as np
import pytest

import span_cases as C
import span_ref as R


def test_the_three_statements_agree():
    seen_empty_t = seen_empty_o = 0
    for seed in range(420):
        t, o, system = C.small_case(seed)
        a = R.span_origins(t, o, system)
        assert a == R.span_enumerate(t, o, system), (seed, t, o, system)
        assert a == R.span_numpy(t, o, system), (seed, t, o, system)
        seen_empty_t += not t
        seen_empty_o += not o
    assert seen_empty_t >= 5 and seen_empty_o >= 5


def test_empty_sides_follow_from_the_definition():
    for system in C.SYSTEMS:
        for f in (R.span_origins, R.span_enumerate, R.span_numpy):
            assert f([1, 2, 3], [], system) == (0, 0, 0)
            assert f([], [1, 2, 3, 1], system) == (0, 0, -4)
            assert f([], [], system) == (0, 0, 0)


def test_exact_substring_is_found_exactly():
    t = [0, 1, 2, 3, 0, 1, 3, 2, 2, 0, 1]
    for f in (R.span_origins, R.span_enumerate, R.span_numpy):
        assert f(t, t[4:8], [8, -4, -7, -7, -3, 0]) == (4, 8, 32)
        assert f(t, t[:3], [8, -4, -7, -7, -3, 0]) == (0, 3, 24)
        assert f(t, t[8:], [8, -4, -7, -7, -3, 0]) == (8, 11, 24)


def test_snap_to_words():
    tr = "ad te levavi  animam meam"
    #     0123456789012345678901234
    assert R.snap_to_words(tr, 6, 12) == (6, 12)            # a whole word stays
    assert R.snap_to_words(tr, 5, 14) == (6, 12)            # a span that starts and ends on spaces loses them
    assert R.snap_to_words(tr, 8, 10) == (6, 12)            # inside one word: outward to the word
    assert R.snap_to_words(tr, 8, 16) == (6, 20)            # cut words at both ends stay whole
    assert R.snap_to_words(tr, 0, 1) == (0, 2) and R.snap_to_words(tr, 22, 25) == (21, 25)
    assert R.snap_to_words(tr, 12, 14) == (14, 14)          # nothing but spaces: empty
    assert R.snap_to_words(tr, 7, 7) == (7, 7)              # an empty span stays empty
    assert R.snap_to_words("", 0, 0) == (0, 0)
    assert R.snap_to_words("abc", 1, 2) == (0, 3)           # no space anywhere


def test_python_interface_refuses_what_the_kernel_cannot_score():
    from text_alignment_amd import textSeqCompare as tsc
    for bad in ([lambda a, b: 1, -1, -1, -1, -1], [8.5, -4, -7, -7, -3, 0], [1, 2, 3]):
        with pytest.raises(ValueError):
            tsc.locate_span(list("abc"), list("b"), bad)
        with pytest.raises(ValueError):
            tsc.locate_spans([(list("abc"), list("b"))], bad)
    with pytest.raises(ValueError):
        tsc.locate_spans([(list("abc"), list("b"))] * 2, [[8, -4, -7, -7, -3, 0]] * 3)
    with pytest.raises(ValueError):
        tsc.locate_spans([(list("abc"), list("b"))] * 2, [[8, -4, -7, -7, -3, 0], [8.5, -4, -7, -7, -3, 0]])


def test_c_interface_refuses_before_any_launch(native):
    lib = native.lib
    big = lib.ta_nw_span_max_m()
    assert 4096 <= big and (big + 2) * 16 + (big + 144) * 2 + 2048 <= 160 * 1024      # the LDS carve fits a CU
    assert lib.ta_nw_span_workspace_bytes(64, 50000, 1000) == 0
    assert lib.ta_nw_span_workspace_bytes(1, 10, big + 1) == native.TA_EINVAL
    assert lib.ta_nw_span_workspace_bytes(1, 1 << 28, 10) == native.TA_EINVAL
    assert lib.ta_nw_span_workspace_bytes(-1, 10, 10) == native.TA_EINVAL
    x = np.zeros(16, dtype=np.int64)                       # host memory: never dereferenced, validation comes first
    ptr = x.ctypes.data

    def call(nprob=1, stride=0, max_n=10, max_m=10, bound=1000, max_param=8, t_start=ptr, out=ptr, t_codes=ptr):
        return lib.ta_nw_span_batch(t_codes, t_start, ptr, ptr, ptr, nprob, ptr, stride, out, max_n, max_m, bound, max_param,
                                    None, 0, None)
    assert call(nprob=0) == native.TA_OK
    assert call(nprob=-1) == native.TA_EINVAL
    assert call(t_start=None) == native.TA_EINVAL and b"null" in lib.ta_last_error()
    assert call(out=None) == native.TA_EINVAL
    assert call(t_codes=None) == native.TA_EINVAL
    assert call(stride=5) == native.TA_EINVAL
    assert call(max_m=big + 1) == native.TA_EINVAL and b"hand-off row" in lib.ta_last_error()
    assert call(max_n=1 << 28) == native.TA_EINVAL and b"origin" in lib.ta_last_error()
    assert call(max_n=-1) == native.TA_EINVAL
    assert call(bound=1 << 23) == native.TA_ERANGE
    assert call(max_param=(1 << 19) + 1) == native.TA_ERANGE
    with pytest.raises(OverflowError):
        native.check(native.TA_ERANGE, "ta_nw_span_batch")
    with pytest.raises(ValueError):
        native.check(native.TA_EINVAL, "ta_nw_span_batch")


# Worst deviation of either end from the planted span over the 24 cases below, as the checker itself gives it
# (printed by the test; the definition, not the kernel, is what is pinned here).
WORST_SEEN = 4


def test_planted_noisy_spans_are_found_by_the_definition():
    """what the feature is for: a page's text (70-80 % of the characters kept, the rest substituted, dropped or
    doubled) is found inside a transcript several times its length, each end within WORST_SEEN + 2 tokens"""
    worst, devs = 0, []
    for seed in range(24):
        keep = 0.70 + 0.10 * (seed % 3) / 2.0
        before = [0, 150, 400][seed % 3] if seed % 5 else 0
        after = [300, 0, 120][seed % 3]
        tr, ocr, (a, b) = C.planted(1000 + seed, before, 160 + 10 * (seed % 4), after, keep)
        t, o = C.codes(tr, ocr)
        i0, i1, _ = R.span_numpy(t, o, C.SYSTEMS[0])
        devs.append((abs(i0 - a), abs(i1 - b)))
        worst = max(worst, abs(i0 - a), abs(i1 - b))
    print("deviations of (i0, i1) from the planted span:", devs, "worst", worst)
    assert worst <= WORST_SEEN + 2
    assert worst == WORST_SEEN       # the figure written above is the one the seeds give
