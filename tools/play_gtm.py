"""Frames of a .gtm stream, played on the device:
python tools/play_gtm.py IN.gtm [--start N --frames N] (--info | --raw OUT.rgb | --y4m OUT.y4m [--chroma 444|422|420jpeg|420mpeg2|mono] [--yuv MODE]
                         | --png OUT_%04d.png [--png-level 0|1] [--png-filter none|adaptive|smaller]
                         | --jpeg OUT_%04d.jpg | --mjpeg OUT.mjpeg [--jpeg-quality 90] [--jpeg-sampling 420|422|444|grey] [--jpeg-restart-rows 1]
                         | --gif OUT.gif [--gif-colours auto|exact|quantise --gif-max-colours 256 --gif-segment 4096 --gif-no-diff]
                         | --webp OUT.webp [--webp-no-diff --webp-palette auto|off --webp-segment 4096])
                         [--size WxH [--filter lanczos|nearest]]

--info prints what the stream says about itself (size, frames, key frames, rate, tiles, palettes, the embedded settings) as JSON;
--raw writes frames [start, start + frames) as packed RGB24, one frame after the other (view with
`ffplay -f rawvideo -pixel_format rgb24 -video_size WxH OUT.rgb`);
--y4m writes them as a Y4M file any player, FFmpeg and this library's OpenInput read: the frames are converted to YUV on the device
(GtmPlayer.ReadYUV) and come to the host as 1 to 3 bytes a pixel.  --yuv: auto (= bt601-limited) bt601-limited bt601-full bt709-limited
bt709-full tiler (444 and mono only); the header says XCOLORRANGE=FULL for the full-range rules and tiler.
--png writes one PNG per frame, named by the pattern with the frame's number: the player's frames stay on the device and are coded there
(stages.png_encode; --png-level 1, the default: deflate on the device, 0: stored blocks).
--jpeg writes one baseline JPEG per frame, --mjpeg the same files one behind another in one file that any player opens: the frames stay on
the device and are coded there (stages.jpeg_encode: libjpeg's bytes; --jpeg-restart-rows 1, the default, writes the restart markers that
let this library's Load decode the files on the device, 0 none).
--gif writes one animated GIF at the stream's rate (stages.gif_encode: exact colour tables where a frame holds at most --gif-max-colours
colours -- a stream of 16 palettes of 16 always does, and the file is lossless -- a median cut where it holds more).
--webp writes one animated lossless WebP at the stream's rate (stages.webp_encode: a VP8L image per frame, exact at any number of colours).
--size WxH (with --raw, --y4m, --png, --jpeg, --mjpeg, --gif and --webp): the frames are scaled on the device to that size before they are delivered (GtmPlayer.SetOutput; --filter
lanczos, the default, or nearest); the Y4M header carries the output size."""
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
g.add_argument("--y4m")
g.add_argument("--png", help="a pattern with one integer field, for instance OUT_%%04d.png")
g.add_argument("--jpeg", help="a pattern with one integer field, for instance OUT_%%04d.jpg")
g.add_argument("--mjpeg")
g.add_argument("--gif")
g.add_argument("--webp")
ap.add_argument("--webp-no-diff", action="store_true", help="code whole frames, not the rectangle that changed")
ap.add_argument("--webp-palette", default="auto", choices=["auto", "off"])
ap.add_argument("--webp-segment", type=int, default=4096, help="coded pixels per separately parsed segment; 0: one per image")
ap.add_argument("--gif-colours", default="auto", choices=["auto", "exact", "quantise"])
ap.add_argument("--gif-max-colours", type=int, default=256)
ap.add_argument("--gif-segment", type=int, default=4096, help="indices per separately coded LZW segment; 0: one per image")
ap.add_argument("--gif-no-diff", action="store_true", help="code whole frames, not the rectangle that changed")
ap.add_argument("--jpeg-quality", type=int, default=90)
ap.add_argument("--jpeg-sampling", default="420", choices=["420", "422", "444", "grey"])
ap.add_argument("--jpeg-restart-rows", type=int, default=1)
ap.add_argument("--png-level", type=int, default=1, choices=[0, 1])
ap.add_argument("--png-filter", default="none", choices=["none", "adaptive", "smaller"])
ap.add_argument("--chroma", default="420jpeg", choices=["444", "422", "420jpeg", "420mpeg2", "mono"])
ap.add_argument("--yuv", default="auto", choices=["auto", "bt601-limited", "bt601-full", "bt709-limited", "bt709-full", "tiler"])
ap.add_argument("--size", help="WxH: the size --raw and --y4m deliver at (default: the stream's own)")
ap.add_argument("--filter", default="lanczos", choices=["lanczos", "nearest"])
args = ap.parse_args()
size = None
if args.size:
    try:
        size = tuple(int(v) for v in args.size.lower().split("x"))
        assert len(size) == 2
    except (ValueError, AssertionError):
        ap.error("--size takes WxH, for instance 1920x1080")
with GtmPlayer(args.input) as p:
    info = p.info()
    if size and not args.info:
        p.SetOutput(size[0], size[1], args.filter)
    if args.info:
        info["keyframe_starts"] = p.KeyFrames().tolist()
        info["settings"] = p.SettingsText()
        print(json.dumps(info))
    elif args.y4m:
        p.Seek(args.start)
        left = (args.frames if args.frames > 0 else info["frames"] - args.start)
        w, h = size if size else (info["tm_w"] * 8, info["tm_h"] * 8)
        full = args.yuv in ("bt601-full", "bt709-full", "tiler")
        with open(args.y4m, "wb") as f:
            f.write(("YUV4MPEG2 W%d H%d F%d:1000000 Ip C%s XCOLORRANGE=%s\n" % (w, h, round(info["fps"] * 1000000), args.chroma, "FULL" if full else "LIMITED")).encode())
            while left > 0:
                planes = p.ReadYUV(min(left, 16), layout=args.chroma, yuv=args.yuv, device=False)
                if planes[0].shape[0] == 0:
                    break
                for i in range(planes[0].shape[0]):
                    f.write(b"FRAME\n")
                    for a in planes:
                        if a is not None:
                            f.write(a[i].tobytes())
                left -= planes[0].shape[0]
    elif args.png:
        from tiler_amd import stages
        p.Seek(args.start)
        left = (args.frames if args.frames > 0 else info["frames"] - args.start)
        at = args.start
        while left > 0:
            fr = p.Read(min(left, 16), device=True)
            if fr.shape[0] == 0:
                break
            for png in stages.png_encode(fr, level=args.png_level, filter=args.png_filter):
                with open(args.png % at, "wb") as f:
                    f.write(png)
                at += 1
            left -= fr.shape[0]
    elif args.jpeg or args.mjpeg:
        from tiler_amd import stages
        p.Seek(args.start)
        left = (args.frames if args.frames > 0 else info["frames"] - args.start)
        at = args.start
        one = open(args.mjpeg, "wb") if args.mjpeg else None
        while left > 0:
            fr = p.Read(min(left, 16), device=True)
            if fr.shape[0] == 0:
                break
            for jpg in stages.jpeg_encode(fr, quality=args.jpeg_quality, sampling=args.jpeg_sampling, restart_rows=args.jpeg_restart_rows):
                if one:
                    one.write(jpg)
                else:
                    with open(args.jpeg % at, "wb") as f:
                        f.write(jpg)
                at += 1
            left -= fr.shape[0]
        if one:
            one.close()
    elif args.gif or args.webp:
        import torch
        from tiler_amd import stages
        p.Seek(args.start)
        left = (args.frames if args.frames > 0 else info["frames"] - args.start)
        parts = []
        while left > 0:
            fr = p.Read(min(left, 16), device=True)
            if fr.shape[0] == 0:
                break
            parts.append(fr.clone())
            left -= fr.shape[0]
        with open(args.gif or args.webp, "wb") as f:  # one file: the frames wait on the device (4 bytes a pixel) and are coded there in the writer's chunks
            if args.webp:
                f.write(stages.webp_encode(torch.cat(parts), info["fps"], diff=not args.webp_no_diff, palette=args.webp_palette, segment_pixels=args.webp_segment))
            else:
                f.write(stages.gif_encode(torch.cat(parts), info["fps"], colours=args.gif_colours, max_colours=args.gif_max_colours, segment_pixels=args.gif_segment,
                                          diff=not args.gif_no_diff))
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
