"""ctypes binding of libta_hip.so (C ABI: include/text_alignment_amd.h).

The HIP library is the product: if it is missing or does not load, importing this module
raises -- there is no CPU fallback anywhere in the package.
"""
import ctypes
import os

# torch first: its wheel bundles the HIP runtime (libamdhip64, soname .so.7).  Loading
# libta_hip.so before torch would pull in /opt/rocm's copy and leave two HIP runtimes in one
# process (kernel launches then fail with "no ROCm-capable device").
import torch  # noqa: F401

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# TA_HIP_LIB: an alternative build of the same library (kernel timing experiments, tools/p2_profile.py)
LIB_PATH = os.environ.get("TA_HIP_LIB") or os.path.join(_HERE, "libta_hip.so")

# every TA_* integer constant of the header, under its own name (TA_OK, TA_EINVAL, TA_NW_*, TA_EVAL_*, ...)
globals().update(_abi.CONSTANTS)


class NativeLibraryError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            "libta_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C text_alignment_amd/csrc`). There is no CPU fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise NativeLibraryError("cannot load %s: %s" % (LIB_PATH, e))
    return _abi.bind(lib)


lib = _load()

EXPORTS = list(_abi.PROTOTYPES)             # every symbol the header declares


class NativeArgumentError(ValueError):
    """TA_EINVAL from the library: the CALLER passed a bad argument -- a programming error, not a property of
    a page's data (sharding.process_shard tells the two apart)"""


def check(rc, what):
    if rc != TA_OK:
        msg = lib.ta_last_error().decode("utf-8", "replace")
        if rc == TA_EINVAL:
            raise NativeArgumentError("%s: %s" % (what, msg))
        if rc == TA_ERANGE:
            raise OverflowError("%s: %s" % (what, msg))
        raise RuntimeError("%s failed (%d): %s" % (what, rc, msg))


def upload_packed(arrays, device):
    """Several small host arrays to the device in ONE asynchronous transfer: packed (16-byte aligned) into a pinned
    buffer, copied non_blocking on torch's current stream, returned as typed views of one device buffer.  A
    `tensor.to(device)` from pageable memory costs ~0.25 ms of host time each; a batch's metadata was ten of them."""
    import numpy as np
    import torch
    arrays = [np.ascontiguousarray(a) for a in arrays]
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.nbytes + 15) // 16 * 16
    host = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    for a, off in zip(arrays, offs):
        if a.nbytes:
            hv[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
    dev = host.to(device, non_blocking=True)
    out = []
    for a, off in zip(arrays, offs):
        t = dev[off:off + a.nbytes].view(getattr(torch, a.dtype.name))
        out.append(t.reshape(a.shape))
    return out


class Download(object):
    """Several device tensors to the host without a wait: a page-locked copy of each, filled non_blocking in the order
    given on torch's current stream, ONE event recorded behind them.  A plain .cpu() issued later would queue behind
    whatever the stream has been given since; a caller with other host work puts it before wait()."""

    def __init__(self, tensors):
        self.host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in tensors]
        for h, t in zip(self.host, tensors):
            h.copy_(t, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def wait(self, waiter=None):
        """the numpy views of the host copies, once the event has passed.  waiter: a callable given the event in place of
        its synchronize() -- a caller that accounts for its waits"""
        if self.event is not None:
            (waiter or torch.cuda.Event.synchronize)(self.event)
            self.event = None
        return [h.numpy() for h in self.host]


download_begin = Download                      # (the name the call sites read by)


def host_copy_pieces(dst_view, pieces, dst_off_bytes):
    """pieces (C-contiguous numpy arrays) -> dst_view (a writable, C-contiguous numpy array, e.g. the view of a page-locked
    tensor) at byte offsets dst_off_bytes[k], in ONE native call that holds no interpreter lock (ta_host_copy_pieces)."""
    import numpy as np
    n = len(pieces)
    if n == 0:
        return
    src = np.fromiter((p.ctypes.data for p in pieces), dtype=np.uint64, count=n)
    nb = np.fromiter((p.nbytes for p in pieces), dtype=np.int64, count=n)
    off = np.ascontiguousarray(dst_off_bytes, dtype=np.int64)
    end = int((off + nb).max())
    if end > dst_view.nbytes or int(off.min()) < 0:
        raise ValueError("a piece does not fit the staging buffer")
    check(lib.ta_host_copy_pieces(dst_view.ctypes.data, src.ctypes.data, off.ctypes.data, nb.ctypes.data, n), "ta_host_copy_pieces")
