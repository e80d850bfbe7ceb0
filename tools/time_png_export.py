"""GeneratePNGs alone on the bench clip:
  python tools/time_png_export.py --dir DIR [--reps 5] [--json OUT.json]      encodes the clip (1280 x 720 x 300, bench.synth_clip, 16 palettes of
                                                                              16) and times GeneratePNGs of the output frames into DIR (a
                                                                              memory-backed directory, so that the disk is not what is timed):
                                                                              wall clock around the call, one warm-up first, then --reps passes
                                                                              at level 0 and at level 1
  python tools/time_png_export.py --dir DIR --against parent ...              the same in child processes, this build and the library
                                                                              tiler_amd/lib/variants/libtilemotion_parent.so (TM_LIB_VARIANT),
                                                                              which is timed at level 0, the only one it has
  python tools/time_png_export.py --dir DIR --only 0|1                        one warm-up and one pass: the program to put behind
                                                                              `rocprofv3 --kernel-trace --stats --`
Every level's files must decode to the same pixels; a sample of them is checked against RenderFrames."""
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

W, H, F = 1280, 720, 300


def encode(out):
    import numpy as np
    import torch
    import bench
    from tiler_amd.encoder import TilingEncoder
    host = bench.synth_clip(np.empty((F, H, W), np.int32), freeze=False)
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    enc.PaletteCount, enc.PaletteSize = 16, 16
    enc.FrameTilingExtendedPaletteUsage = False
    enc.MotionPredictRadius = 0
    enc.OutputFileName = out
    enc.SetVideo(W, H, 24.0, F)
    enc.SetFramesDevice(torch.from_numpy(host).cuda())
    for step in range(7):  # everything but Save
        enc.Run(step)
    return enc


def has_levels(enc):
    return hasattr(enc, "SetPngOptions") and getattr(enc._L, "tm_set_png_options", None) is not None


def export_once(enc):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enc.GeneratePNGs(False)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, (enc.ExportStats() if has_levels(enc) else None)


def check_sample(enc, base):
    """frames 0, 149 and 299 as Pillow reads them against RenderFrames"""
    import numpy as np
    from PIL import Image
    for f in (0, F // 2 - 1, F - 1):
        a = np.asarray(Image.open("%s_%04d.png" % (base, f)).convert("RGB")).astype(np.uint32)
        want = enc.RenderFrames(f, 1, device=False)[0] & 0xFFFFFF
        assert np.array_equal((a[..., 0] << 16) | (a[..., 1] << 8) | a[..., 2], want), f


def child(args):
    base = os.path.join(args.dir, "export")
    enc = encode(base + ".gtm")
    levels = ([args.only] if args.only is not None else [0, 1]) if has_levels(enc) else [0]
    out = dict(lib=os.environ.get("TM_LIB_VARIANT", ""), reps=args.reps, levels={})
    for level in levels:
        if has_levels(enc):
            enc.SetPngOptions(level=level)
        export_once(enc)  # warm-up: code objects, the pool, the directory's pages
        runs = [export_once(enc) for _ in range(1 if args.only is not None else max(args.reps, 1))]
        check_sample(enc, base)
        c = dict(wall_ms=[r[0] for r in runs], file_bytes=sum(os.path.getsize(p) for p in glob.glob(base + "_*.png")))
        if runs[-1][1]:
            c["split_ms"] = {k: statistics.median(r[1][k] for r in runs) for k in ("ms_device", "ms_write", "ms_wall")}
            c["filter"] = runs[-1][1]["filter"]
        out["levels"][str(level)] = c
    enc.close()
    return out


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--against", help="a library variant (tiler_amd/lib/variants/libtilemotion_<name>.so) to time beside this build")
    ap.add_argument("--only", type=int, choices=[0, 1])
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    if args.child or not args.against:
        result = child(args)
    else:
        result = dict(clip="%d x %d x %d, bench.synth_clip, 16 palettes of 16, output frames" % (W, H, F), reps=args.reps)
        for lib in (args.against, ""):  # a fresh process each: a process loads one library
            env = dict(os.environ)
            env.pop("TM_LIB_VARIANT", None)
            if lib:
                env["TM_LIB_VARIANT"] = lib
            tmp = os.path.join(args.dir, "child.json")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--dir", args.dir, "--reps", str(args.reps), "--json", tmp, "--child"], env=env, timeout=900)
            result[lib or "this_build"] = json.load(open(tmp))["levels"]
    for levels in ([result["levels"]] if "levels" in result else [v for k, v in result.items() if isinstance(v, dict)]):
        for c in levels.values():
            if isinstance(c.get("wall_ms"), list) and not args.child:
                c["wall_ms"] = spread(c["wall_ms"])
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
