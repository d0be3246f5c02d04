"""What harvesting adds to a page pass: 64 synthetic pages x 20 lines of 150 .. 420 columns
(already-normalised rows, a random 96-class model, transcripts drawn from a small Latin vocabulary) through the first
stages of `alignToOCR.process_batch` as one chunk -- recognise, characters, abbreviations, ONE aligner launch, the
alignment columns back on the host -- once WITHOUT the harvest (the stages alone) and once WITH it
(`harvest.harvest_pages`: the same stages, the two harvest launches, the table's download and the per-line result
objects), same inputs.  Wall milliseconds, medians of --passes passes after a warm-up pass each, and their difference;
besides, HIP events around `harvest_alignment` alone on the resident batch (the two launches and the metadata upload).
Writes profiles/harvest_time.json; no threshold is set here.  The model's OCR is noise against these transcripts, so
nearly every line is rejected: the time does not depend on that, the accepted fraction says nothing about real pages.

    python tools/harvest_time.py [--pages 64] [--passes 10] [--out profiles/harvest_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

VOCAB = ("dominus deus meus alleluia gloria patri et filio spiritui sancto sicut erat in principio nunc semper saecula "
         "saeculorum amen laudate eum omnes gentes quoniam confirmata est super nos misericordia eius veritas manet").split()


def synthetic_pages(npages, nlines, seed):
    from text_alignment_amd import page as page_mod
    rng = np.random.default_rng(seed)
    pages, trs = [], []
    for _ in range(npages):
        strips = []
        for k in range(nlines):
            w = int(rng.integers(150, 421))
            xs = np.zeros((w + 32, 48), dtype=np.float32)
            xs[16:16 + w] = (rng.random((w, 48)) < 0.15) * rng.random((w, 48))
            strips.append(page_mod.Strip(offset_x=40 + int(rng.integers(0, 30)), offset_y=100 + 120 * k, height=60,
                                         width=2 * w, prepared=xs))
        pages.append(page_mod.PreparedPage((2200, 3300), (2200, 3300), 0, strips, [130 + 120 * k for k in range(nlines + 1)]))
        trs.append(" ".join(VOCAB[int(i)] for i in rng.integers(0, len(VOCAB), size=6 * nlines)))
    return pages, trs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--lines", type=int, default=20)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "harvest_time.json"))
    args = ap.parse_args()
    import torch
    from text_alignment_amd import alignToOCR as atocr, harvest, ocr
    model = ocr.LineModel.random(7001, no=96)
    rec = ocr.LineRecognizer(model)
    pages, trs = synthetic_pages(args.pages, args.lines, 4100)
    params = [8, -1, -9, -9, -4, -4]
    kept = {}

    def stages():
        chunk = atocr.PageChunk(rec, pages, trs, params, atocr.parallel)
        chunk.launch()
        chunk.host_ahead()
        chunk.align()
        return chunk

    def without():
        kept["ops"] = stages().columns()

    def with_harvest():
        kept["res"] = harvest.harvest_pages(pages, trs, rec, params, 0.9)

    def wall(fn):
        fn()                                                           # warm-up: allocator, code objects
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return {"ms": ms, "median_ms": statistics.median(ms)}
    out = {"pages": args.pages, "lines_per_page": args.lines, "passes": args.passes, "device": torch.cuda.get_device_name(0),
           "precision": ocr.DEFAULT_PRECISION}
    out["without_harvest"] = wall(without)
    out["with_harvest"] = wall(with_harvest)
    out["difference_ms"] = out["with_harvest"]["median_ms"] - out["without_harvest"]["median_ms"]
    res = kept["res"]
    assert all(np.array_equal(a, b) for a, b in zip(res.ops, kept["ops"]))          # the same alignments both ways
    out["lines"] = len(res)
    out["accepted_lines_of_this_noise_model"] = sum(1 for ln in res.lines if ln.reason == 0)
    out["alignment_columns"] = int(sum(len(o) for o in res.ops))

    # the harvest call alone, on a batch that stays resident
    chunk = stages()
    batch = chunk.nw
    chunk.columns()
    o_line, _, T = chunk.line_table()
    o_line = np.concatenate(o_line)
    cls = np.concatenate([harvest.transcript_classes(model.codec, t) for t in trs])
    stream = atocr._nw_stream(rec.device)
    ev = []
    with torch.cuda.stream(stream):
        for k in range(args.passes + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tables = harvest.harvest_alignment(batch, o_line, res.line_first, cls, T, 0.9)
            e1.record()
            e1.synchronize()
            if k:
                ev.append(e0.elapsed_time(e1))
        assert np.array_equal(tables.host()["table"], res.table)
    out["harvest_alignment_events"] = {"ms": ev, "median_ms": statistics.median(ev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "ms"}) for k, v in out.items()}))


if __name__ == "__main__":
    main()
