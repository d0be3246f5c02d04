"""Training augmentation on the device (csrc/ta_distort.hip): random elastic distortion of raw text-line strips, the
`rdistort` of ocropy's `ocropus-linegen` / the ocrodeg recipe -- two gaussian-smoothed noise fields scaled to a maximal
displacement, the strip resampled bilinearly through them.  The arithmetic is DESIGN.md section 14.4 (PARITY UNPINNED,
like the rest of section 14; the checker of record is tests/distort_ref.py).  Raw strips in, distorted strips out, in
one packed buffer the normaliser (lineest_gpu) takes as one slice; there is no host path.
"""
import numpy as np
import torch

from . import _native
from . import lineest_gpu
from . import page as page_mod

DISTORT = 3.0               # maximal displacement in pixels and smoothing sigma: rdistort's defaults (unpinned)
DSIGMA = 10.0
MAX_H = _native.TA_DISTORT_MAX_H
MAX_RADIUS = _native.TA_DISTORT_MAX_RADIUS


def check_params(distort, dsigma):
    """(distort, dsigma) as floats; ValueError for what ta_line_distort would refuse, before the device is touched"""
    distort, dsigma = float(distort), float(dsigma)
    if not (0 < distort < 1e9) or not (0 < dsigma < float("inf")):
        raise ValueError("distort and dsigma must be positive")
    if int(4.0 * dsigma + 0.5) > MAX_RADIUS:
        raise ValueError("dsigma %g: the gaussian's radius exceeds %d" % (dsigma, MAX_RADIUS))
    return distort, dsigma


def distort_strips(strips, distort=DISTORT, dsigma=DSIGMA, seed=0, first_counter=0, device="cuda", want_fields=False):
    """strips: what lineest_gpu.measure_strips_begin takes -- 2-D uint8 images (white background) as host arrays, device
    tensors or page.DeviceStrip.  Returns the distorted strips, same sizes, as a list of page.DeviceStrip into ONE packed
    buffer; with want_fields, (that list, per strip a float64 device tensor (2, h, w): the row and the column
    displacements in pixels).  Strip k draws its noise with key `seed` and counter `first_counter + k` (both 64 bits),
    so a strip's result does not depend on its neighbours in the batch.  Enqueues on torch's current stream and waits
    for nothing."""
    distort, dsigma = check_params(distort, dsigma)
    seed, first_counter = int(seed), int(first_counter)
    if not 0 <= seed < 2 ** 64 or not 0 <= first_counter < 2 ** 64:
        raise ValueError("seed and first_counter are unsigned 64-bit numbers")
    strips = list(strips)
    n = len(strips)
    if n == 0:
        return ([], []) if want_fields else []
    dev = torch.device(device)
    hh, ww, pix_off, spans, on_device = lineest_gpu._strip_sizes(strips, dev)
    if int(hh.max()) > MAX_H:
        raise ValueError("a strip of %d rows is taller than the %d the distortion takes" % (int(hh.max()), MAX_H))
    if int((hh.astype(np.int64) * ww).max()) > 2 ** 31 - 1:
        raise ValueError("a strip has more than 2^31 - 1 pixels")
    lib = _native.lib
    total = int(pix_off[-1])
    with torch.cuda.device(dev):
        d_pix = lineest_gpu._pack_strips(strips, hh, ww, pix_off, spans, on_device, dev)
        gw, _ = lineest_gpu._gauss_weights(dsigma)
        counters = ((first_counter + np.arange(n, dtype=object)) % 2 ** 64).astype(np.uint64).view(np.int64)
        d_pix_off, d_hh, d_ww, d_counters, d_gw = _native.upload_packed([pix_off[:-1].copy(), hh, ww, counters, gw], dev)
        ws_bytes = int(lib.ta_line_distort_workspace_bytes(n, total))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        fields = torch.empty(2 * total, dtype=torch.float64, device=dev) if want_fields else None
        here = torch.cuda.current_stream(dev)
        _native.check(lib.ta_line_distort(
            d_pix.data_ptr(), d_pix_off.data_ptr(), d_hh.data_ptr(), d_ww.data_ptr(), d_counters.data_ptr(), n,
            hh.ctypes.data, ww.ctypes.data, distort, dsigma, seed, d_gw.data_ptr(), ws.data_ptr(), ws_bytes,
            out.data_ptr(), fields.data_ptr() if want_fields else None, here.cuda_stream), "ta_line_distort")
        # what the kernels read may belong to another stream's allocator (a caller's strips, the upload's buffers)
        for t in (d_pix, d_pix_off, ws):
            t.record_stream(here)
    res = [page_mod.DeviceStrip(out, int(pix_off[k]), int(hh[k]), int(ww[k])) for k in range(n)]
    if not want_fields:
        return res
    return res, [fields[2 * int(pix_off[k]):2 * int(pix_off[k + 1])].view(2, int(hh[k]), int(ww[k])) for k in range(n)]
