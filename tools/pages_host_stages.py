"""The calling thread's stages of ONE process_batch pass, in order, with their wall time (a stage's time INCLUDES any
wait for the device or for the page threads inside it): where the host side of the chunk pipeline spends a call.
python tools/pages_host_stages.py [npages] [--images | --raw | --rows pinned|device]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools import pages_bench as pb, switches
from text_alignment_amd import alignToOCR as atocr, page as page_mod

switches.apply()
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 64
rec = pb.make_recognizer()
if "--images" in sys.argv:
    pages, trs = [pb.RawPage(pb.make_page_image(9100 + k)) for k in range(n)], [pb.page_meta(100 + k)[1] for k in range(n)]
elif "--rows" in sys.argv:
    pages, trs, _blocks = pb.make_pages_in_blocks([100 + k for k in range(n)], sys.argv[sys.argv.index("--rows") + 1])
else:
    raw = "--raw" in sys.argv
    pages, trs = zip(*[pb.make_page(100 + k + (5000 if raw else 0), raw=raw) for k in range(n)])
log = []


def wrap(owner, name, label=None):
    fn = getattr(owner, name)

    def timed(*a, **kw):
        t0 = time.perf_counter()
        try:
            return fn(*a, **kw)
        finally:
            log.append((label or name, t0, time.perf_counter()))
    setattr(owner, name, timed)


STAGES = ("PageChunk", "launch", "host_ahead", "align", "finish")       # (PageChunk: its constructor, the first stage's host part)
for name, label in zip(("__init__",) + STAGES[1:], STAGES):
    wrap(atocr.PageChunk, name, label)
wrap(atocr, "find_lines_all")
wrap(page_mod, "prepared_lines")
for name in ("prepare", "complete", "run"):
    wrap(type(rec), name, "rec." + name)
for _ in range(3):
    atocr.process_batch(list(pages), list(trs), rec, pb.PARAMS)
torch.cuda.synchronize()
for rep in range(2):
    del log[:]
    w0 = atocr.WAIT_SECONDS[0]
    t0 = time.perf_counter()
    atocr.process_batch(list(pages), list(trs), rec, pb.PARAMS)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    print("pass %d: %.2f ms, of which waiting for the device in the later stages %.2f ms" % (rep, 1e3 * (t1 - t0), 1e3 * (atocr.WAIT_SECONDS[0] - w0)))
    outer = [e for e in log if e[0] in STAGES]
    for name, a, b in sorted(outer, key=lambda e: e[1]):
        inner = ", ".join("%s %.2f" % (nm, 1e3 * (y - x)) for nm, x, y in log if nm not in STAGES and x >= a and y <= b)
        print("   %7.2f ms  %-16s %6.2f ms   %s" % (1e3 * (a - t0), name, 1e3 * (b - a), inner))
    print("   totals: " + ", ".join("%s %.2f" % (s, 1e3 * sum(b - a for nm, a, b in outer if nm == s)) for s in STAGES))
