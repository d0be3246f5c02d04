"""ta_forced_align_omit_lines -- the omission-tolerant forced alignment whose line list lies on the device -- on the cases
of tests/forced_omit_cases.py: the layout that tests/test_forced_omit_lines_sim.py (the host build of
csrc/ta_forced_omit.hip) and tests/test_forced_omit_lines_gpu.py (the real kernel) share.

The layout is forced_lines_cases.pack's -- the case's lines scattered over more chunk lines than there are texts (acc_line a
permutation with holes), caps equal to L and above it, slots behind the filled ones, everything poisoned -- with the
workspace pieces sized by ta_forced_omit_workspace_bytes of the CAPS.
"""
import numpy as np

import forced_lines_cases as LC
import forced_omit_cases as OC
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = LC.POISON32, LC.POISON64, LC.POISON_BYTE
INPUTS, OUTPUTS = LC.INPUTS, LC.OUTPUTS
untouched = LC.untouched


def bind(lib):
    OC.bind(lib)
    return _abi.bind(lib, ["ta_forced_align_omit_lines"])


class _Sizes(object):
    """forced_lines_cases.pack (and forced_cases.pack under it) ask their library for the size of a line's workspace
    piece: the tolerant kernel's here"""

    def __init__(self, lib):
        self.ta_forced_workspace_bytes = lib.ta_forced_omit_workspace_bytes


def pack(lib, lines, no, **kw):
    return LC.pack(_Sizes(lib), lines, no, **kw)


def call(lib, pk, ptr, omit, stream=None, **over):
    """ta_forced_align_omit_lines on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to
    replace"""
    a = dict(nlines_all=pk.nlines_all, nslots=pk.nslots, no=pk.no, rows=pk.rows, label_cap=pk.nlabels,
             T_all_host=pk.T_all_host, Lcap_host=pk.Lcap_host, omit_q=omit, workspace=ptr("ws"), workspace_bytes=pk.ws_bytes)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    for name in ("T_all_host", "Lcap_host"):
        if isinstance(a[name], np.ndarray):
            a[name] = a[name].ctypes.data
    return lib.ta_forced_align_omit_lines(*[a[k] for k in INPUTS], a["nlines_all"], a["nslots"], a["no"], a["rows"],
                                          a["label_cap"], a["T_all_host"], a["Lcap_host"], a["omit_q"], a["workspace"],
                                          a["workspace_bytes"], a["frames"], a["score"], a["status"], stream)


def refusals(pk):
    """forced_lines_cases.refusals plus omit_q out of range"""
    return LC.refusals(pk) + [("omit_q = -1", -1, dict(omit_q=-1)), ("omit_q = 2^26 + 1", -1, dict(omit_q=(1 << 26) + 1))]
