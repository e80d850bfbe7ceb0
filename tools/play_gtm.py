"""Frames of a .gtm stream, played on the device: python tools/play_gtm.py IN.gtm [--start N --frames N] (--info | --raw OUT.rgb)

--info prints what the stream says about itself (size, frames, key frames, rate, tiles, palettes, the embedded settings) as JSON;
--raw writes frames [start, start + frames) as packed RGB24, one frame after the other (view with
`ffplay -f rawvideo -pixel_format rgb24 -video_size WxH OUT.rgb`)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tiler_amd.player import GtmPlayer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("input")
ap.add_argument("--start", type=int, default=0)
ap.add_argument("--frames", type=int, default=0, help="0: to the end")
g = ap.add_mutually_exclusive_group(required=True)
g.add_argument("--info", action="store_true")
g.add_argument("--raw")
args = ap.parse_args()
with GtmPlayer(args.input) as p:
    info = p.info()
    if args.info:
        info["keyframe_starts"] = p.KeyFrames().tolist()
        info["settings"] = p.SettingsText()
        print(json.dumps(info))
    else:
        p.Seek(args.start)
        left = (args.frames if args.frames > 0 else info["frames"] - args.start)
        with open(args.raw, "wb") as f:
            while left > 0:
                fr = p.Read(min(left, 16), device=False)  # 0x00RRGGBB
                if fr.shape[0] == 0:
                    break
                rgb = np.stack([(fr >> 16) & 255, (fr >> 8) & 255, fr & 255], axis=-1).astype(np.uint8)
                f.write(rgb.tobytes())
                left -= fr.shape[0]
