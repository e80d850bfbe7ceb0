"""The player against reload + render on the bench clip:
  python tools/time_player.py --dir DIR [--reps 5] [--json OUT.json]      makes the two streams (1280 x 720 x 300, motion radius 32 and 0) in DIR
                                                                          unless they are there, and times both ways on both
  python tools/time_player.py --dir DIR --only old|player --motion 0|1    one untimed pass of one way on one stream: the program to put behind
                                                                          `rocprofv3 --kernel-trace --stats --` for the kernels' own times
  python tools/time_player.py --dir DIR --yuv rgb32|nv12|p010|... --to host|device [--motion 0|1] [--reps 7] [--json OUT.json]
                                                                          the read leg: all frames of one stream as RGB32
                                                                          (tm_player_read) or as YUV planes (tm_player_read_yuv) into device memory
                                                                          or page-locked host memory; wall times and the bytes that cross PCIe.
                                                                          With --only player: one untimed pass, for rocprofv3.
                                                                          --size WxH --filter lanczos|nearest: the frames are delivered at that
                                                                          size (GtmPlayer.SetOutput)
(a) the old way: tm_reload_gtm + tm_render_frames of all frames into device memory;  (b) tm_player_open + tm_player_read of all frames into
device memory, with the worker thread and (TM_PLAYER_NO_WORKER=1) without.  Wall times are medians of --reps runs after one warm-up, with
min and max; the player's own split (decode, parse, upload, wait for the worker, launches) and its time to the first frame are its Timings()."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from tiler_amd.encoder import TilingEncoder  # noqa: E402
from tiler_amd.player import GtmPlayer  # noqa: E402

W, H, F = 1280, 720, 300


def make_stream(path, radius):
    host = bench.synth_clip(np.empty((F, H, W), np.int32), freeze=False)
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    enc.PaletteCount, enc.PaletteSize = 16, 16
    enc.FrameTilingExtendedPaletteUsage = False
    enc.MotionPredictRadius = radius
    enc.OutputFileName = path
    enc.SetVideo(W, H, 24.0, F)
    frames = torch.from_numpy(host).cuda()
    enc.SetFramesDevice(frames)
    enc.Run()
    maps = enc.TileMaps()
    pred = int(((maps["Flags"] >> 2) & 1).sum())
    info = dict(keyframes=len(enc.KeyFrames()), tiles=enc.counts()["tiles"], predicted_items=pred, items=int(maps.size), bytes=os.path.getsize(path))
    enc.close()
    return info


def old_way(path, out):
    t0 = time.perf_counter()
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    enc.SetVideo(W, H, 24.0, F)
    enc.ReloadGTM(path)
    t1 = time.perf_counter()
    from tiler_amd._lib import check, c_void_p
    check(enc._L.tm_render_frames(c_void_p(enc._h), 0, F, 0, c_void_p(out.data_ptr()), 1))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    enc.close()
    return dict(wall_ms=(t2 - t0) * 1e3, reload_ms=(t1 - t0) * 1e3, render_ms=(t2 - t1) * 1e3)


def player_way(path, out):
    t0 = time.perf_counter()
    with GtmPlayer(path) as p:
        t1 = time.perf_counter()
        got = p.Read(F, out=out)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert got.shape[0] == F
        r = p.Timings()
        i = p.info()
    r.update(wall_ms=(t2 - t0) * 1e3, open_ms=(t1 - t0) * 1e3, read_ms=(t2 - t1) * 1e3, host_bytes=i["host_bytes"], device_bytes=i["device_bytes"])
    return r


def yuv_leg(path, layout, to, reps, size=None, filter="lanczos"):
    """all frames of the stream read `reps` times after one warm-up, each time by a fresh player: wall ms of open + read, of the read alone,
    and the bytes the read sends over PCIe (0 for a device destination)"""
    from tiler_amd import yuv_out
    W, H = size if size else (globals()["W"], globals()["H"])
    if layout == "rgb32":
        out = torch.empty((F, H, W), dtype=torch.int32, device="cuda") if to == "device" else torch.empty((F, H, W), dtype=torch.int32, pin_memory=True)
        nbytes = out.numel() * 4
    else:
        words = yuv_out.layout_of(layout)[1] != yuv_out.U8
        shapes = yuv_out.plane_shapes(layout, F, H, W)
        make = (lambda s: torch.empty(s, dtype=torch.int16 if words else torch.uint8, device="cuda")) if to == "device" else \
               (lambda s: torch.empty(s, dtype=torch.int16 if words else torch.uint8, pin_memory=True))
        out = tuple(None if s is None else make(s) for s in shapes)
        nbytes = sum(a.numel() * a.element_size() for a in out if a is not None)

    def once():
        t0 = time.perf_counter()
        with GtmPlayer(path) as p:
            if size:
                p.SetOutput(W, H, filter)
            t1 = time.perf_counter()
            if layout == "rgb32":
                got = p.Read(F, device=True, out=out) if to == "device" else p.Read(F, device=False, out=out.numpy().view(np.uint32))
                n = got.shape[0]
            else:
                n = p.ReadYUV(F, layout=layout, device=to == "device", out=out)[0].shape[0]
            torch.cuda.synchronize()
            t2 = time.perf_counter()
        assert n == F
        return dict(wall_ms=(t2 - t0) * 1e3, read_ms=(t2 - t1) * 1e3)

    once()
    if reps <= 0:
        return None
    r = summarise([once() for _ in range(reps)])
    r.update(layout=layout, to=to, reps=reps, size="%dx%d" % (W, H), filter=filter if size else None, bytes_written=nbytes, pcie_bytes=0 if to == "device" else nbytes, lib=os.environ.get("TM_LIB_VARIANT", ""))
    return r


def summarise(runs):
    out = {}
    for k in runs[0]:
        v = [r[k] for r in runs]
        out[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--only", choices=["old", "player"])
    ap.add_argument("--motion", type=int, default=1)
    ap.add_argument("--yuv", help="the read leg: rgb32, or a layout of GtmPlayer.ReadYUV (nv12, p010, 420, ...)")
    ap.add_argument("--to", choices=["host", "device"], default="device")
    ap.add_argument("--size", help="WxH: the read leg delivers at this size")
    ap.add_argument("--filter", default="lanczos", choices=["lanczos", "nearest"])
    args = ap.parse_args()
    size = tuple(int(v) for v in args.size.lower().split("x")) if args.size else None
    if size and not args.yuv:
        ap.error("--size belongs to the read leg: give --yuv rgb32 or a layout")
    os.makedirs(args.dir, exist_ok=True)
    paths = {1: os.path.join(args.dir, "bench_motion32.gtm"), 0: os.path.join(args.dir, "bench_motion0.gtm")}
    if args.yuv:
        if not os.path.exists(paths[args.motion]):
            make_stream(paths[args.motion], 32 if args.motion else 0)
        r = yuv_leg(paths[args.motion], args.yuv, args.to, 0 if args.only else args.reps, size, args.filter)
        if r is not None:
            print(json.dumps(r))
            if args.json:
                with open(args.json, "w") as f:
                    f.write(json.dumps(r) + "\n")
        return
    out = torch.empty((F, H, W), dtype=torch.int32, device="cuda")
    if args.only:
        (old_way if args.only == "old" else player_way)(paths[args.motion], out)
        return
    result = dict(clip="%d x %d x %d, bench.synth_clip, 16 palettes of 16" % (W, H, F), reps=args.reps, streams={})
    for motion, radius in ((1, 32), (0, 0)):
        made = make_stream(paths[motion], radius) if not os.path.exists(paths[motion]) else dict(bytes=os.path.getsize(paths[motion]))
        res = dict(stream=made)
        old_way(paths[motion], out)  # warm-up: code objects, the pool
        ref = out.clone()
        res["old"] = summarise([old_way(paths[motion], out) for _ in range(args.reps)])
        player_way(paths[motion], out)
        assert torch.equal(out, ref), "the player's frames differ from reload + render"
        res["player"] = summarise([player_way(paths[motion], out) for _ in range(args.reps)])
        os.environ["TM_PLAYER_NO_WORKER"] = "1"
        res["player_no_worker"] = summarise([player_way(paths[motion], out) for _ in range(args.reps)])
        del os.environ["TM_PLAYER_NO_WORKER"]
        result["streams"]["motion32" if motion else "motion0"] = res
        del ref
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
