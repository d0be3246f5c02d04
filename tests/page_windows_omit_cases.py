"""What tests/test_page_windows_omit_sim.py (the host build) and tests/test_page_windows_omit_gpu.py (the real kernel) share
on top of tests/page_windows_cases.py: the call of ta_page_windows_omit (csrc/ta_page_windows_omit.hip; DESIGN.md section
14.17), the expected answers -- forced.page_scope_eligibility(..., omit=True) -- and the pages at the two limits.

The limit pages need windows of at most 1023 characters, so a page of 2^20 characters needs 1026 lines (cores of 1023
characters that tile the text, margin 0); ONE line would have the window [0, n) and be PAGE_WINDOWS, which stands in front
of PAGE_TOO_LONG.  The tables stay small all the same: t_class is the only large array.
"""
import numpy as np

import page_windows_cases as C
from text_alignment_amd import _abi

TOO_LONG = _abi.CONSTANTS["TA_PAGE_SCOPE_TOO_LONG"]
MAX_CHARS, MAX_FRAMES = 1 << 20, 1 << 25


def bind(lib):
    return _abi.bind(lib, ["ta_page_windows_omit"])


def want(pages, margin):
    from text_alignment_amd import forced
    return [forced.page_scope_eligibility(pg["plain"], pg["status"], pg["classes"], pg["rows"], pg["T"], margin, omit=True)
            for pg in pages]


def call(lib, pk, ptr, m, stream=None, **over):
    a = dict(npages=pk.npages, nlines=pk.nlines, t_len=pk.t_len, margin=m)
    for name in C.INPUTS + C.OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    return lib.ta_page_windows_omit(a["table"], a["h_status"], a["line_first"], a["t_off"], a["t_class"], a["T"], a["plain"],
                                    a["npages"], a["nlines"], a["t_len"], a["margin"], a["lo"], a["hi"], a["reason"], stream)


def long_text(n):
    """a page of n characters of class 1 whose lines' cores of 1023 characters tile the text (margin 0): one frame a line"""
    starts = np.arange(0, n, C.MAX_TARGET)
    rows = [[0, int(s), int(min(C.MAX_TARGET, n - s))] for s in starts]
    return C.page(rows, n, T=np.ones(len(rows), np.int32), classes=np.ones(n, np.int32))


def many_frames(total):
    """a page of `total` frames in lines of 5 000 (and one shorter), a character per line (margin 1)"""
    full, rest = divmod(total, 5000)
    T = [5000] * full + ([rest] if rest else [])
    rows, n = C.chain(len(T), L=1, gap=0)
    return C.page(rows, n, T=T, classes=np.ones(n, np.int32))


def limit_cases():
    """(name, margin, pages, reasons)"""
    wide = [[0, 0, 1024], [0, 1024, MAX_CHARS - 1024 + 1]]            # a window of 1024 characters AND 2^20 + 1 characters
    return [("2^20 characters", 0, [long_text(MAX_CHARS), long_text(MAX_CHARS + 1)], [0, TOO_LONG]),
            ("2^25 frames", 1, [many_frames(MAX_FRAMES), many_frames(MAX_FRAMES + 1)], [0, TOO_LONG]),
            ("WINDOWS in front of TOO_LONG", 0, [C.page(wide, MAX_CHARS + 1, T=[5, 5], classes=np.ones(MAX_CHARS + 1, np.int32))],
             [5])]
