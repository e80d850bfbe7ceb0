"""GenerateJPEGs alone on the bench clip, beside GeneratePNGs at level 1:
  python tools/time_jpeg_export.py --dir DIR [--reps 7] [--json OUT.json]     encodes the clip (1280 x 720 x 300, bench.synth_clip, 16 palettes of
                                                                              16) and times exports of the output frames into DIR (a
                                                                              memory-backed directory, so that the disk is not what is timed):
                                                                              wall clock around the call, one warm-up of each first, then
                                                                              --reps rounds that alternate GeneratePNGs at level 1, GenerateJPEGs
                                                                              with restart_rows 1 and with restart_rows 0 (quality 90, 4:2:0)
  python tools/time_jpeg_export.py --dir DIR --against parent ...             the PNG leg in child processes of the library
                                                                              tiler_amd/lib/variants/libtilemotion_parent.so (TM_LIB_VARIANT),
                                                                              the JPEG legs in child processes of this build, the two taking
                                                                              turns (parent, this build, parent, this build) with the rounds
                                                                              split between the turns
  python tools/time_jpeg_export.py --dir DIR --load                           also reads the exported sequences back: OpenInput + Run(esLoad) of
                                                                              each, TM_JPEG_DECODE=device and =host in turn
  python tools/time_jpeg_export.py --dir DIR --only png1|jpeg_r1|jpeg_r0      one warm-up and one pass: the program to put behind
                                                                              `rocprofv3 --kernel-trace --stats --`
Medians with min-max.  A sample of the JPEG files is checked against the host twin of RenderFrames, and with Pillow, where it is
installed, against libjpeg."""
import argparse
import glob
import io
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.time_png_export import F, H, W, encode  # noqa: E402

LEGS = {"png1": None, "jpeg_r1": dict(quality=90, sampling="420", restart_rows=1), "jpeg_r0": dict(quality=90, sampling="420", restart_rows=0)}


def has_jpeg(enc):
    return hasattr(enc, "SetJpegOptions") and getattr(enc._L, "tm_set_jpeg_options", None) is not None


def export_once(enc, leg, base):
    import torch
    for n in glob.glob(base + "_*.png") + glob.glob(base + "_*.jpg"):
        os.remove(n)
    if leg == "png1":
        enc.SetPngOptions(level=1)
    else:
        enc.SetJpegOptions(**LEGS[leg])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if leg == "png1":
        enc.GeneratePNGs(False)
    else:
        enc.GenerateJPEGs(False)
    wall = (time.perf_counter() - t0) * 1e3
    st = enc.ExportStats() if leg == "png1" else enc.JpegExportStats()
    names = glob.glob(base + ("_*.png" if leg == "png1" else "_*.jpg"))
    assert len(names) == F and st["file_bytes"] == sum(os.path.getsize(n) for n in names)
    return wall, st


def check_sample(enc, leg, base):
    """frames 0, 149 and 299 against the host twin of RenderFrames and against Pillow"""
    import numpy as np
    from tiler_amd import stages
    for f in (0, F // 2 - 1, F - 1):
        data = open("%s_%04d.jpg" % (base, f), "rb").read()
        frame = enc.RenderFrames(f, 1, device=False)
        assert [data] == stages.jpeg_encode_host(frame, **LEGS[leg]), f
        try:
            from PIL import Image
        except ImportError:
            continue
        px = frame[0]
        rgb = np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], -1).astype(np.uint8)
        out = io.BytesIO()
        Image.fromarray(rgb, "RGB").save(out, "JPEG", quality=90, subsampling=2, restart_marker_rows=LEGS[leg]["restart_rows"])
        assert out.getvalue() == data, f


def load_back(base, passes):
    """OpenInput + Run(esLoad) of the sequence in DIR, device and host in turn; one warm-up each"""
    from tiler_amd.encoder import TilingEncoder, TEncoderStep as S
    ms, encs, stats = {"device": [], "host": []}, {}, {}
    for where in ms:
        encs[where] = TilingEncoder()
        encs[where].LoadDefaultSettings()
        encs[where].InputFileName = base + "_%.4d.jpg"
    try:
        for p in range(passes + 1):
            for where in ms:
                os.environ["TM_JPEG_DECODE"] = where
                t0 = time.perf_counter()
                encs[where].OpenInput()
                encs[where].Run(S.esLoad)
                ms[where].append((time.perf_counter() - t0) * 1e3)
    finally:
        os.environ.pop("TM_JPEG_DECODE", None)
    for where in ms:
        stats[where] = dict(ms=ms[where][1:], input_stats=encs[where].InputStats())
        encs[where].close()
    return stats


def child(args):
    base = os.path.join(args.dir, "export")
    enc = encode(base + ".gtm")
    legs = [args.only] if args.only else [l for l in (args.legs.split(",") if args.legs else LEGS) if l == "png1" or has_jpeg(enc)]
    out = dict(lib=os.environ.get("TM_LIB_VARIANT", ""), reps=args.reps, legs={l: dict(wall_ms=[], ms_device=[], ms_write=[]) for l in legs})
    for leg in legs:
        export_once(enc, leg, base)  # warm-up: code objects, the pool, the directory's pages
    for _ in range(1 if args.only else max(args.reps, 1)):
        for leg in legs:  # in turn, so that a drift of the machine falls on all
            wall, st = export_once(enc, leg, base)
            c = out["legs"][leg]
            c["wall_ms"].append(wall); c["ms_device"].append(st["ms_device"]); c["ms_write"].append(st["ms_write"])
            c["file_bytes"] = st["file_bytes"]
    for leg in legs:
        if leg != "png1":
            export_once(enc, leg, base)
            check_sample(enc, leg, base)
            if args.load:
                out["legs"][leg]["load_back"] = load_back(base, args.reps)
    enc.close()
    return out


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def summarise(legs):
    for c in legs.values():
        for k in ("wall_ms", "ms_device", "ms_write"):
            if isinstance(c.get(k), list) and c[k]:
                c[k] = spread(c[k])
        for where in c.get("load_back", {}).values():
            where["ms"] = spread(where["ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json")
    ap.add_argument("--against", help="a library variant (tiler_amd/lib/variants/libtilemotion_<name>.so) whose GeneratePNGs at level 1 is timed beside this build's GenerateJPEGs")
    ap.add_argument("--only", choices=list(LEGS))
    ap.add_argument("--load", action="store_true")
    ap.add_argument("--legs", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    if args.child or not args.against:
        result = child(args)
        if not args.child:
            summarise(result["legs"])
    else:
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
            cmd = [sys.executable, os.path.abspath(__file__), "--dir", args.dir, "--reps", str(reps), "--json", tmp, "--child", "--legs", "png1" if lib else "jpeg_r1,jpeg_r0"]
            subprocess.check_call(cmd + (["--load"] if args.load and not lib and not merged.get("this_build", {}).get("jpeg_r1", {}).get("load_back") else []), env=env, timeout=1100)
            got = json.load(open(tmp))["legs"]
            result["order"].append(lib or "this_build")
            into = merged.setdefault(lib or "this_build", {})
            for leg, c in got.items():
                m = into.setdefault(leg, dict(wall_ms=[], ms_device=[], ms_write=[]))
                for k in ("wall_ms", "ms_device", "ms_write"):
                    m[k] += c[k]
                m["file_bytes"] = c["file_bytes"]
                if "load_back" in c:
                    m["load_back"] = c["load_back"]
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
