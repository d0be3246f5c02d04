"""The layout tests/test_forced_page_omit_gated_sim.py (the host build) and tests/test_forced_page_omit_gated_gpu.py (the real
kernel) drive ta_forced_align_pages_omit_gated with, on the pages of
tests/forced_page_omit_cases.py and the answers of tests/forced_page_omit_ref.py.

Slots, packing, poison and the check are forced_page_gated_cases' -- (page, gate, cap), pieces sized by the page's CAP, not
a byte of a passed-over page's pieces touched -- with the pieces sized by ta_forced_page_omit_gated_workspace_bytes.
"""
import numpy as np

import forced_page_gated_cases as G
import forced_page_omit_ref as R

POISON32, POISON64, POISON_BYTE = G.POISON32, G.POISON64, G.POISON_BYTE
SKIPPED, MAX_TARGET = G.SKIPPED, G.MAX_TARGET
INPUTS, OUTPUTS, HOST = G.INPUTS, G.OUTPUTS, G.HOST
slots, check = G.slots, G.check


def bind(lib):
    from text_alignment_amd import _abi
    return _abi.bind(lib, ["ta_forced_page_omit_gated_workspace_bytes", "ta_forced_align_pages_omit_gated"])


class _Sizes(object):
    """forced_page_gated_cases.pack sizes the pieces with ta_forced_page_gated_workspace_bytes: here the entry with omission's"""
    def __init__(self, lib):
        self.ta_forced_page_gated_workspace_bytes = lib.ta_forced_page_omit_gated_workspace_bytes


def pack(lib, slot_list, no):
    return G.pack(_Sizes(lib), slot_list, no)


def call(lib, pk, ptr, omit, stream=None, **over):
    """ta_forced_align_pages_omit_gated on pk's arrays, as forced_page_gated_cases.call"""
    a = dict(npages=pk.npages, nlines=pk.nlines, no=pk.no, rows=pk.rows, nlabels=pk.nlabels, T_host=pk.T,
             line_first_host=pk.line_first, lab_off_host=pk.lab_off, cap_host=pk.cap, workspace=ptr("ws"),
             workspace_bytes=pk.ws_bytes, omit_q=omit)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    keep = []
    for name in HOST:
        if isinstance(a[name], np.ndarray):
            keep.append(np.ascontiguousarray(a[name]))
            a[name] = keep[-1].ctypes.data
    return lib.ta_forced_align_pages_omit_gated(
        a["probs"], a["row_off"], a["T"], a["line_first"], a["lo"], a["hi"], a["labels"], a["lab_off"], a["ws_off"],
        a["gate"], a["cap"], a["npages"], a["nlines"], a["no"], a["rows"], a["nlabels"], a["T_host"], a["line_first_host"],
        a["lab_off_host"], a["cap_host"], a["omit_q"], a["workspace"], a["workspace_bytes"], a["frames"], a["score"],
        a["status"], stream)


def want(slot_list, omit):
    """[(status, score, frames)] per slot: SKIPPED for a gated page, else the checker's"""
    return [(SKIPPED, None, None) if g != 0 else R.answer(*pg, omit) for pg, g, _ in slot_list]
