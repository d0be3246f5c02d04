"""Times the device page preprocessing + line finding (csrc/ta_preproc.hip) against the host
checker (oracle/preproc_ref.py) on a synthetic page, and prints a sha256 over what the device made of it (the two
planes, the angle, the strips' boxes and pixels): two builds of the library, or the two labellers
(TA_PP_LABEL_PIXELS=1, tools/switches.py), are compared by it.  python tools/preproc_bench.py [nlines]"""
import hashlib
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import numpy as np
    import torch
    from test_preprocessing import _synthetic_page
    from text_alignment_amd import preproc_gpu as G
    from oracle import preproc_ref as H
    from tools import switches
    switches.apply()
    nlines = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    img, _ = _synthetic_page(nlines, angle=1.5)
    G.find_lines(img)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        out = G.find_lines(img)
    torch.cuda.synchronize()
    dev = (time.perf_counter() - t0) / 3
    t1 = time.perf_counter()
    H.find_lines(img)
    host = time.perf_counter() - t1
    sha = hashlib.sha256()
    for plane in out[:2]:
        sha.update(np.ascontiguousarray(plane.ink).tobytes())
    sha.update(repr(float(out[2])).encode())
    for s in out[3]:
        sha.update(repr((s.offset_x, s.offset_y, s.height, s.width)).encode())
        sha.update(np.ascontiguousarray(s.pixels).tobytes())
    print({"page": img.shape, "strips": len(out[3]), "device_s": dev, "host_s_one_core": host, "sha256": sha.hexdigest()})


if __name__ == "__main__":
    main()
