"""GenerateGIF alone on the bench clip, beside GeneratePNGs at level 1 and GenerateMJPEG:
  python tools/time_gif_export.py --dir DIR [--reps 7] [--json OUT.json]     encodes the clip (1280 x 720 x 300, bench.synth_clip, 16 palettes of
                                                                             16: at most 256 colours a frame, the exact path) and times exports
                                                                             of the output frames into DIR (a memory-backed directory, so that
                                                                             the disk is not what is timed): wall clock around the call, one
                                                                             warm-up of each first, then --reps rounds that alternate
                                                                             GeneratePNGs at level 1, GenerateMJPEG and GenerateGIF at
                                                                             segment_pixels 4096, 16384, 65536 and 0; then the flat 16-colour
                                                                             clip (1280 x 720 x 60 of 8 x 8 blocks, every 16th block changing a
                                                                             frame) through stages.gif_encode at the same segment sizes
  python tools/time_gif_export.py --dir DIR --against parent ...             the PNG and MJPEG legs in child processes of the library
                                                                             tiler_amd/lib/variants/libtilemotion_parent.so (TM_LIB_VARIANT),
                                                                             the GIF legs in child processes of this build, the two taking turns
                                                                             (parent, this build, parent, this build) with the rounds split
  python tools/time_gif_export.py --dir DIR --only png1|mjpeg|gif_16384|...  one warm-up and one pass: the program to put behind
                                                                             `rocprofv3 --kernel-trace --stats --`
  python tools/time_gif_export.py --sizes                                    no device: the host twin's file sizes of the flat clip at the four
                                                                             segment sizes (they are the device's)
Medians with min-max; per-stage milliseconds from GifExportStats.  Frames 0, 149 and 299 of every GIF are read back with the project's reader
and held to RenderFrames."""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.time_png_export import F, H, W, encode  # noqa: E402

SEGMENTS = (4096, 16384, 65536, 0)
LEGS = ["png1", "mjpeg"] + ["gif_%d" % s for s in SEGMENTS]
STAGES = ("ms_colours", "ms_tables", "ms_lzw", "ms_emit", "ms_device", "ms_write")


def has_gif(enc):
    return hasattr(enc, "SetGifOptions") and getattr(enc._L, "tm_set_gif_options", None) is not None


def flat_clip(nf=60):
    """1280 x 720 x nf in 16 colours: 8 x 8 blocks, every 16th block takes a new colour each frame"""
    import numpy as np
    rng = np.random.default_rng(42)
    pal = np.array([(i * 0x111111) & 0xFFFFFF for i in range(16)], np.uint32)
    blocks = rng.integers(0, 16, (H // 8, W // 8))
    out = np.empty((nf, H, W), np.uint32)
    for f in range(nf):
        change = rng.random(blocks.shape) < 1 / 16
        blocks = np.where(change, rng.integers(0, 16, blocks.shape), blocks)
        out[f] = pal[blocks].repeat(8, axis=0).repeat(8, axis=1)
    return out


def export_once(enc, leg, base):
    import torch
    for n in glob.glob(base + "_*.png") + glob.glob(base + ".mjpeg") + glob.glob(base + ".gif"):
        os.remove(n)
    if leg == "png1":
        enc.SetPngOptions(level=1)
    elif leg == "mjpeg":
        enc.SetJpegOptions()
    else:
        enc.SetGifOptions(segment_pixels=int(leg[4:]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if leg == "png1":
        enc.GeneratePNGs(False)
    elif leg == "mjpeg":
        enc.GenerateMJPEG(base + ".mjpeg", False)
    else:
        enc.GenerateGIF(base + ".gif", False)
    wall = (time.perf_counter() - t0) * 1e3
    st = enc.ExportStats() if leg == "png1" else enc.JpegExportStats() if leg == "mjpeg" else enc.GifExportStats()
    return wall, st


def check_sample(enc, base):
    import numpy as np
    from tiler_amd import stages
    file = open(base + ".gif", "rb").read()
    for f in (0, F // 2 - 1, F - 1):
        shown, status = stages.gif_decode_host(file, 0, f + 1)
        assert status == [0] * (f + 1) and np.array_equal(shown[f], enc.RenderFrames(f, 1, device=False)[0] & 0xFFFFFF), f


def flat_legs(reps):
    import torch
    from tiler_amd import stages
    frames = flat_clip()
    dev = torch.from_numpy(frames.view("int32")).cuda()
    out = {}
    for s in SEGMENTS:
        stages.gif_encode(dev, 25.0, segment_pixels=s)
    for _ in range(reps):
        for s in SEGMENTS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = stages.gif_encode(dev, 25.0, segment_pixels=s, full=True)
            c = out.setdefault("flat_gif_%d" % s, dict(wall_ms=[], file_bytes=r["bytes"], **{k: [] for k in STAGES if k in r["stats"]}))
            c["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            for k in STAGES:
                if k in c:
                    c[k].append(r["stats"][k])
    return out


def child(args):
    base = os.path.join(args.dir, "export")
    enc = encode(base + ".gtm")
    legs = [args.only] if args.only else [l for l in (args.legs.split(",") if args.legs else LEGS) if not l.startswith("gif") or has_gif(enc)]
    out = dict(lib=os.environ.get("TM_LIB_VARIANT", ""), reps=args.reps, legs={})
    for leg in legs:
        export_once(enc, leg, base)  # warm-up: code objects, the pool, the directory's pages
    for _ in range(1 if args.only else max(args.reps, 1)):
        for leg in legs:  # in turn, so that a drift of the machine falls on all
            wall, st = export_once(enc, leg, base)
            c = out["legs"].setdefault(leg, dict(wall_ms=[], **{k: [] for k in STAGES if k in st}))
            c["wall_ms"].append(wall)
            for k in STAGES:
                if k in st:
                    c[k].append(st[k])
            c["file_bytes"] = st["file_bytes"]
            for k in ("frames_exact", "frames_quantised", "segments"):
                if k in st:
                    c[k] = st[k]
            if leg.startswith("gif") and len(c["wall_ms"]) == 1:
                check_sample(enc, base)
    enc.close()
    if not args.only and any(l.startswith("gif") for l in legs):
        out["legs"].update(flat_legs(max(args.reps, 1)))
    return out


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def summarise(legs):
    for c in legs.values():
        for k in ("wall_ms",) + STAGES:
            if isinstance(c.get(k), list) and c[k]:
                c[k] = spread(c[k])


def sizes():
    from tiler_amd import stages
    frames = flat_clip()
    return {"flat_gif_%d" % s: len(stages.gif_encode_host(frames, 25.0, segment_pixels=s)) for s in SEGMENTS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json")
    ap.add_argument("--against", help="a library variant (tiler_amd/lib/variants/libtilemotion_<name>.so) whose GeneratePNGs and GenerateMJPEG are timed beside this build's GenerateGIF")
    ap.add_argument("--only", choices=LEGS)
    ap.add_argument("--sizes", action="store_true")
    ap.add_argument("--legs", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.sizes:
        result = sizes()
    elif not args.dir:
        ap.error("--dir is required")
    elif args.child or not args.against:
        os.makedirs(args.dir, exist_ok=True)
        result = child(args)
        if not args.child:
            summarise(result["legs"])
    else:
        os.makedirs(args.dir, exist_ok=True)
        result = dict(clip="%d x %d x %d, bench.synth_clip, 16 palettes of 16, output frames" % (W, H, F), reps=args.reps, order=[])
        merged = {}
        first = (args.reps + 1) // 2
        for lib, reps in ((args.against, first), ("", first), (args.against, args.reps - first), ("", args.reps - first)):  # a process loads one library
            if reps <= 0:
                continue
            env = dict(os.environ)
            env.pop("TM_LIB_VARIANT", None)
            if lib:
                env["TM_LIB_VARIANT"] = lib
            tmp = os.path.join(args.dir, "child.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--dir", args.dir, "--reps", str(reps), "--json", tmp, "--child", "--legs",
                   "png1,mjpeg" if lib else ",".join(l for l in LEGS if l.startswith("gif"))]
            subprocess.check_call(cmd, env=env, timeout=1100)
            got = json.load(open(tmp))["legs"]
            result["order"].append(lib or "this_build")
            into = merged.setdefault(lib or "this_build", {})
            for leg, c in got.items():
                m = into.setdefault(leg, {})
                for k, v in c.items():
                    if isinstance(v, list):
                        m[k] = m.get(k, []) + v
                    else:
                        m[k] = v
        for legs in merged.values():
            summarise(legs)
        result.update(merged)
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
