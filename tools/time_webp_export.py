"""GenerateWebP alone on the bench clip, beside GeneratePNGs at level 1 and GenerateGIF:
  python tools/time_webp_export.py --dir DIR [--reps 7] [--json OUT.json]   encodes the clip (1280 x 720 x 300, bench.synth_clip, 16 palettes
                                                                            of 16) and times exports of the output frames into DIR (a
                                                                            memory-backed directory, so that the disk is not what is timed):
                                                                            wall clock around the call, one warm-up of each first, then
                                                                            --reps rounds that alternate GeneratePNGs at level 1, GenerateGIF
                                                                            and GenerateWebP at segment_pixels 4096, 16384, 65536 and 0
  python tools/time_webp_export.py --dir DIR --only png1|gif|webp_16384|... one warm-up and one pass: the program to put behind
                                                                            `rocprofv3 --kernel-trace --stats --`
Medians with min-max; per-stage milliseconds from WebpExportStats.  Frames 0, 149 and 299 of the first WebP are read back with Pillow and
held to RenderFrames."""
import argparse
import glob
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.time_png_export import F, H, W, encode  # noqa: E402

SEGMENTS = (4096, 16384, 65536, 0)
LEGS = ["png1", "gif"] + ["webp_%d" % s for s in SEGMENTS]
STAGES = ("ms_colours", "ms_match", "ms_parse", "ms_codes", "ms_emit", "ms_tables", "ms_lzw", "ms_device", "ms_write")
COUNTS = ("frames_indexed", "segments", "tokens", "matches")


def export_once(enc, leg, base):
    import torch
    for n in glob.glob(base + "_*.png") + glob.glob(base + ".gif") + glob.glob(base + ".webp"):
        os.remove(n)
    if leg == "png1":
        enc.SetPngOptions(level=1)
    elif leg == "gif":
        enc.SetGifOptions()
    else:
        enc.SetWebpOptions(segment_pixels=int(leg[5:]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if leg == "png1":
        enc.GeneratePNGs(False)
    elif leg == "gif":
        enc.GenerateGIF(base + ".gif", False)
    else:
        enc.GenerateWebP(base + ".webp", False)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, enc.ExportStats() if leg == "png1" else enc.GifExportStats() if leg == "gif" else enc.WebpExportStats()


def check_sample(enc, base):
    import numpy as np
    from PIL import Image
    im = Image.open(io.BytesIO(open(base + ".webp", "rb").read()))
    assert im.n_frames == F
    for f in (0, F // 2 - 1, F - 1):
        im.seek(f)
        a = np.asarray(im.convert("RGB")).astype(np.uint32)
        assert np.array_equal(a[..., 0] << 16 | a[..., 1] << 8 | a[..., 2], enc.RenderFrames(f, 1, device=False)[0] & 0xFFFFFF), f


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json")
    ap.add_argument("--only", choices=LEGS)
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    base = os.path.join(args.dir, "export")
    enc = encode(base + ".gtm")
    legs = [args.only] if args.only else LEGS
    out = {}
    checked = False
    for leg in legs:
        export_once(enc, leg, base)  # warm-up: code objects, the pool, the directory's pages
    for _ in range(1 if args.only else max(args.reps, 1)):
        for leg in legs:  # in turn, so that a drift of the machine falls on all
            wall, st = export_once(enc, leg, base)
            c = out.setdefault(leg, dict(wall_ms=[], **{k: [] for k in STAGES if k in st}))
            c["wall_ms"].append(wall)
            for k in STAGES:
                if k in st:
                    c[k].append(st[k])
            c["file_bytes"] = st["file_bytes"]
            for k in COUNTS:
                if k in st:
                    c[k] = st[k]
            if leg.startswith("webp") and not checked and not args.only:
                check_sample(enc, base)
                checked = True
    enc.close()
    for c in out.values():
        for k in ("wall_ms",) + STAGES:
            if isinstance(c.get(k), list) and c[k]:
                c[k] = spread(c[k])
    text = json.dumps(dict(clip="%d x %d x %d, bench.synth_clip, 16 palettes of 16, output frames" % (W, H, F), reps=args.reps, legs=out), indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
