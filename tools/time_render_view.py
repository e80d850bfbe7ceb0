"""Render's views on the bench clip (1280 x 720 x 300, motion off, 16 palettes):
  python tools/time_render_view.py [--passes 7] [--json OUT.json]   wall times (medians with min and max, after a warm-up, each pass ended by a
                                                                    device synchronise) of RenderFrames and of the views into device memory
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_render_view.py --passes 5
                                                                    the same calls untimed by the host: the kernels' own times are the trace's
Copied into a checkout of the commit before the views (whose library has none), only RenderFrames runs, so that k_render_output can be
measured there in the same visit.  The default view is checked against RenderFrames bit for bit before anything is timed."""
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
from tiler_amd._lib import lib  # noqa: E402
from tiler_amd.encoder import TilingEncoder  # noqa: E402

W, H, F = 1280, 720, 300


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    has_views = hasattr(lib(), "tm_render_view_frames")
    host = bench.synth_clip(np.empty((F, H, W), np.int32), freeze=False)
    frames = torch.from_numpy(host).cuda()
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    enc.PaletteCount, enc.PaletteSize = 16, 16
    enc.FrameTilingExtendedPaletteUsage = False
    enc.MotionPredictRadius = 0
    enc.SetVideo(W, H, 24.0, F)
    enc.SetFramesDevice(frames)
    enc.Run()
    c = enc.counts()
    calls = {"render_frames": lambda: enc.RenderFrames(), "render_frames_input": lambda: enc.RenderFrames(input=True)}
    if has_views:
        calls.update({
            "view_default": lambda: enc.RenderView(device=True),
            "view_undithered": lambda: enc.RenderView(dithered=False, device=True),
            "view_gamma": lambda: enc.RenderView(gamma=0.6, device=True),
            "view_palette_7": lambda: enc.RenderView(palette=7, device=True),
            "view_input": lambda: enc.RenderView(page="input", device=True),
            "tile_pages_one_launch": lambda: enc.RenderTilePages(device=True),
        })
        assert torch.equal(enc.RenderView(device=True), enc.RenderFrames()), "the default view is not RenderFrames"
        assert torch.equal(enc.RenderView(page="input", device=True), enc.RenderFrames(input=True))
    res = dict(clip=[W, H, F], tiles=c["tiles"], items=F * c["tm_w"] * c["tm_h"], tile_pages=enc.TilePageCount() if has_views else None,
               library="with views" if has_views else "without views", passes=a.passes, wall_ms={})
    for name, fn in calls.items():
        out = fn()  # warm: code object, pool
        torch.cuda.synchronize()
        del out
        t = []
        for _ in range(a.passes):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
            del out
        res["wall_ms"][name] = dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4))
    enc.close()
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
