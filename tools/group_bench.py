"""Device group measurements for DESIGN.md section 7 (tm_set_devices): not bench.py.

  python tools/group_bench.py                 Run(esAll) on the 720p x 300, 16-palette clip, motion prediction off and on: the single encoder
                                              against a group of two shards on device 0 (a rehearsal: expected slower), and against one
                                              shard per device when two or more are visible; the outputs must be identical
  python tools/group_bench.py --probe-only    the group all-reduce alone (tm_probe_group_allreduce) at 25 KB and 17 MB, for a rocprofv3 run

One JSON line per measurement on stdout; exit status 1 when a group's output differs from the single encoder's.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def probe(devices, nbytes, iters):
    from tiler_amd._lib import lib, check
    L = lib()
    arr = (ctypes.c_int * len(devices))(*devices)
    us = ctypes.c_double()
    check(L.tm_probe_group_allreduce(arr, len(devices), int(nbytes), int(iters), ctypes.byref(us)))
    return us.value


def encode(frames, devices, motion, palettes, repeat):
    import torch
    from tiler_amd.encoder import TilingEncoder
    F, H, W = frames.shape
    enc = TilingEncoder()
    if devices is not None:
        enc.SetDevices(devices)
    enc.LoadDefaultSettings()
    enc.PaletteCount = palettes
    enc.PaletteSize = 16
    enc.FrameTilingExtendedPaletteUsage = False
    enc.MotionPredictRadius = motion
    enc.SetVideo(W, H, 24.0, F)
    enc.SetFramesDevice(frames)
    enc.Run()  # warm-up: pools, tables, code objects
    times = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.Run()
        times.append(time.perf_counter() - t0)
    hdr, pal, rgb = enc.Tiles()
    out = dict(tilemaps=enc.TileMaps(), hdr=hdr, pal=pal, rgb=rgb, palettes=enc.Palettes(), keyframes=enc.KeyFrames())
    stats = enc.CollectiveStats()
    enc.close()
    return min(times) * 1e3, out, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--palettes", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--probe-only", action="store_true")
    args = ap.parse_args()
    from tiler_amd._lib import lib
    ndev = lib().tm_device_count()
    for nbytes, what in ((25 * 1024, "one Lloyd iteration"), (17 * 1024 * 1024, "a Q-sized int32 tile-map merge")):
        iters = 200 if nbytes < 1 << 20 else 50
        for devs in ([0, 0], [0, 1]) if ndev >= 2 else ([0, 0],):
            print(json.dumps(dict(measure="group_allreduce", bytes=nbytes, what=what, devices=devs, us_per_call=round(probe(devs, nbytes, iters), 1))), flush=True)
    if args.probe_only:
        return 0
    import torch
    sys.path.insert(0, ROOT)
    from bench import synth_clip
    host = torch.empty((args.frames, args.height, args.width), dtype=torch.int32, pin_memory=True)
    synth_clip(host.numpy(), freeze=False)
    frames = host.cuda()
    torch.cuda.synchronize()
    bad = 0
    for motion in (0, 32):
        ms, want, _ = encode(frames, None, motion, args.palettes, args.repeat)
        print(json.dumps(dict(measure="run_all", motion_radius=motion, devices="single", ms=round(ms, 1))), flush=True)
        groups = [[0, 0]] + ([list(range(ndev))] if ndev >= 2 else [])
        for devs in groups:
            ms, got, stats = encode(frames, devs, motion, args.palettes, args.repeat)
            same = all(np.array_equal(got[k], want[k]) for k in want)
            bad += not same
            print(json.dumps(dict(measure="run_all", motion_radius=motion, devices=devs, ms=round(ms, 1), identical=same,
                                  collective_bytes=stats["bytes"])), flush=True)
        if ndev < 2:
            print(json.dumps(dict(measure="run_all", motion_radius=motion, devices="one shard per device", ms="not measured",
                                  note="%d device visible" % ndev)), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
