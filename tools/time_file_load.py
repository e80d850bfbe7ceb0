"""Wall time of Load from a Y4M file against Load of the same clip as RGB32 in page-locked host memory, and of the same clip lent as YUV planes.

    python tools/time_file_load.py [--mode file|host|both|yuv|rgb|png|jpeg|gif|all] [--frames 300 --width 1280 --height 720] [--scaling 1.0] [--passes 7] [--dir /dev/shm]

The clip is bench.py's (SURVEY.md 8d's generator).  `file`: it is written as a 4:2:0 Y4M into --dir (memory-backed by default, so that the
figure is the pipeline's and not a disk's) and every pass is OpenInput + Run(esLoad).  `host`: the RGB32 clip sits in pinned memory and every
pass is SetFramesHost + Run(esLoad) -- the path a caller had before Load could read a file; it uses no call newer than that, so the same
script times an older build of the library.  `yuv` (`all`: every leg): the planes are lent with SetFramesYUV and every pass is SetFramesYUV +
Run(esLoad) -- (d) planar 4:2:0 in page-locked host memory, (e) NV12 in device memory, (f) P010 in device memory (the bytes in the high
bits of 10-bit samples).  `rgb` (and `all`): the clip is lent with SetFramesRGB and every pass is SetFramesRGB + Run(esLoad) -- rgb24 and bgra in
page-locked host memory, rgb24 and gbrp 10-bit in device memory, rgb24 in device memory at Scaling 0.5; the device legs also time the
conversion alone (stages.rgb_to_rgb32) between two events.  `png` (not part of `all`): the clip is written into --dir as a PNG sequence, once by
Pillow at its defaults and once by this library's level-1 export, and every pass is OpenInput + Run(esLoad) under TM_PNG_DECODE=host and
=device; with --png-keep the sequences stay in --dir for the next call (an older build of the library, loaded with TM_LIB_VARIANT, reads them
under `host` alone: --png-where host).  `jpeg` (not part of `all`): the clip is written into --dir by Pillow as a JPEG sequence (quality 90, 4:2:0), once
without restart markers and once with an interval of one MCU row, and the passes alternate between TM_JPEG_DECODE=device and =host, every
pass OpenInput + Run(esLoad); --jpeg-blocks N,M,... times sequences with restart intervals of N, M, ... MCUs instead.  `gif` (not part of `all`; meant for a GIF-like size such as --frames 120
--width 480 --height 270): two animated GIFs are written into --dir by Pillow -- the clip in 256 colours, and a flat, cartoon-like one of the same
size (plain areas, moving shapes, 16 colours) -- and the passes alternate between TM_GIF_DECODE=device and =host, every pass OpenInput + Run(esLoad).
One warm-up pass, then the median of --passes passes with their spread; one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rgb_to_yuv420(frames):
    """BT.601 limited range, chroma as the mean of each 2x2 block (centred: C420jpeg)"""
    r, g, b = ((frames >> s) & 255 for s in (16, 8, 0))
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    u = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    v = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
    h, w = frames.shape
    sub = lambda c: (c.reshape(h // 2, 2, w // 2, 2).sum((1, 3)) + 2) >> 2
    return y.astype(np.uint8), sub(u).astype(np.uint8), sub(v).astype(np.uint8)


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), passes=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["file", "host", "both", "yuv", "rgb", "png", "jpeg", "gif", "all"], default="both")
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--scaling", type=float, default=1.0)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--png-where", default="host,device", help="the TM_PNG_DECODE settings --mode png times")
    ap.add_argument("--jpeg-blocks", default="", help="--mode jpeg: time these restart intervals (MCUs, comma separated) instead of the two standard sequences")
    ap.add_argument("--jpeg-writer", default="pillow", choices=["pillow", "library"],
                    help="--mode jpeg: who writes the sequences: Pillow, or this library's exporter on the device (stages.jpeg_encode: the same bytes; restart_rows 0 and 1 only)")
    ap.add_argument("--png-keep", action="store_true", help="--mode png: leave the sequences in --dir, and use those that are there")
    args = ap.parse_args()
    import torch
    from bench import synth_clip
    from tiler_amd.encoder import TilingEncoder, TEncoderStep as S
    F, H, W = args.frames, args.height, args.width
    assert W % 2 == 0 and H % 2 == 0
    host = torch.empty((F, H, W), dtype=torch.int32, pin_memory=True)
    clip = synth_clip(host.numpy(), freeze=True)
    out = dict(clip="%dx%dx%d" % (W, H, F), scaling=args.scaling, rgb32_bytes=F * H * W * 4, yuv420_bytes=F * H * W * 3 // 2)

    if args.mode in ("host", "both", "all"):
        enc = TilingEncoder()
        enc.LoadDefaultSettings()
        enc.SetVideo(W, H, 24.0, F)
        ms = []
        for p in range(args.passes + 1):
            enc.SetFramesHost(host)
            t0 = time.perf_counter()
            enc.Run(S.esLoad)
            ms.append((time.perf_counter() - t0) * 1e3)
        enc.close()
        out["load_host_rgb32"] = stats(ms[1:])

    if args.mode in ("yuv", "all"):
        from tiler_amd.encoder import TChroma, TSamples
        planes = [torch.empty(shape, dtype=torch.uint8, pin_memory=True) for shape in ((F, H, W), (F, H // 2, W // 2), (F, H // 2, W // 2))]
        for i in range(F):
            for dst, src in zip(planes, rgb_to_yuv420(clip[i].astype(np.int64))):
                dst[i] = torch.from_numpy(src)
        y_dev = planes[0].cuda()
        uv_dev = torch.stack([planes[1], planes[2]], -1).reshape(F, H // 2, W).cuda()  # NV12: (U, V) pairs
        y10, uv10 = (t.to(torch.int16) << 8 for t in (y_dev, uv_dev))                  # P010: the sample in the high 10 bits of the word
        legs = (("load_yuv420_host_pinned", planes, dict(samples=TSamples.u8, depth=8)),
                ("load_nv12_device", (y_dev, uv_dev), dict(samples=TSamples.u8, depth=8)),
                ("load_p010_device", (y10, uv10), dict(samples=TSamples.u16High, depth=10)))
        for name, lent, fmt in legs:
            enc = TilingEncoder()
            enc.LoadDefaultSettings()
            enc.Scaling = args.scaling
            ms = []
            for p in range(args.passes + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                info = enc.SetFramesYUV(*lent, chroma=TChroma.c420jpeg, fps=24.0, **fmt)
                enc.Run(S.esLoad)
                ms.append((time.perf_counter() - t0) * 1e3)
            enc.close()
            out[name] = dict(stats(ms[1:]), video=info)

    if args.mode in ("rgb", "all"):
        from tiler_amd import stages
        px = torch.from_numpy(clip.view(np.uint8).reshape(F, H, W, 4))  # little-endian 0xAARRGGBB: bytes B, G, R, A
        rgb24 = torch.empty((F, H, W, 3), dtype=torch.uint8, pin_memory=True)
        rgb24.copy_(px[..., [2, 1, 0]])
        bgra = host.view(torch.uint8).view(F, H, W, 4)  # (the yardstick's own memory, lent as it lies)
        rgb24_dev = rgb24.cuda()
        gbrp10 = (rgb24_dev.permute(0, 3, 1, 2)[:, [1, 2, 0]].to(torch.int16) << 2).contiguous()  # the bytes in 10-bit samples, low bits of the word
        legs = (("load_rgb24_host_pinned", rgb24, "rgb24", None, args.scaling), ("load_bgra_host_pinned", bgra, "bgra", None, args.scaling),
                ("load_rgb24_device", rgb24_dev, "rgb24", None, args.scaling), ("load_gbrp10_device", gbrp10, "gbrp", 10, args.scaling),
                ("load_rgb24_device_half", rgb24_dev, "rgb24", None, 0.5))
        for name, lent, layout, depth, scaling in legs:
            enc = TilingEncoder()
            enc.LoadDefaultSettings()
            enc.Scaling = scaling
            ms = []
            for p in range(args.passes + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                info = enc.SetFramesRGB(lent, layout, fps=24.0, depth=depth)
                enc.Run(S.esLoad)
                ms.append((time.perf_counter() - t0) * 1e3)
            enc.close()
            out[name] = dict(stats(ms[1:]), video=info)
            if lent.is_cuda:  # the conversion alone, between two events on the stream (the tables of a scaled pass are made inside: see kernel_ms of a trace)
                size, kms = (info["width"], info["height"]), []
                dst = torch.empty((F, size[1], size[0]), dtype=torch.int32, device="cuda")
                for p in range(args.passes + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    stages.rgb_to_rgb32(lent, layout, size=size, depth=depth, out=dst)
                    e1.record()
                    torch.cuda.synchronize()
                    kms.append(e0.elapsed_time(e1))
                out[name]["convert_events"] = stats(kms[1:])
                del dst

    if args.mode == "png":
        from PIL import Image
        for writer in ("pillow", "own"):
            stem = os.path.join(args.dir, "time_png_load_%s_%dx%dx%d" % (writer, W, H, F))
            names = ["%s_%04d.png" % (stem, i) for i in range(F)]
            try:
                if not all(os.path.exists(n) for n in names):
                    if writer == "pillow":
                        for i in range(F):
                            fr = clip[i]
                            Image.fromarray(np.stack([(fr >> 16) & 255, (fr >> 8) & 255, fr & 255], -1).astype(np.uint8), "RGB").save(names[i], "PNG")
                    else:
                        enc = TilingEncoder()
                        enc.LoadDefaultSettings()
                        enc.OutputFileName = stem + ".gtm"
                        enc.SetVideo(W, H, 24.0, F)
                        enc.SetFramesHost(host)
                        enc.Run(S.esLoad)
                        enc.SetPngOptions(level=1)
                        enc.GeneratePNGs(input=True)
                        enc.close()
                leg = dict(file_bytes=sum(os.path.getsize(n) for n in names))
                for where in args.png_where.split(","):
                    os.environ["TM_PNG_DECODE"] = where
                    enc = TilingEncoder()
                    enc.LoadDefaultSettings()
                    enc.InputFileName = stem + "_%.4d.png"
                    ms = []
                    for p in range(args.passes + 1):
                        t0 = time.perf_counter()
                        info = enc.OpenInput()
                        enc.Run(S.esLoad)
                        ms.append((time.perf_counter() - t0) * 1e3)
                    leg[where] = dict(stats(ms[1:]), video=info)
                    if hasattr(enc._L, "tm_get_input_stats"):
                        leg[where]["input_stats"] = enc.InputStats()
                    enc.close()
                out["load_png_" + writer] = leg
            finally:
                os.environ.pop("TM_PNG_DECODE", None)
                if not args.png_keep:
                    for n in names + [stem + ".txt"]:
                        if os.path.exists(n):
                            os.remove(n)

    if args.mode == "jpeg":
        from PIL import Image
        legs = [("plain", {}), ("restart_rows", {"restart_marker_rows": 1})]
        if args.jpeg_blocks:  # further legs: a restart interval of so many MCUs
            legs = [("restart_%s_mcus" % b, {"restart_marker_blocks": int(b)}) for b in args.jpeg_blocks.split(",")]
        for name, opts in legs:
            stem = os.path.join(args.dir, "time_jpeg_load_%s_%d_%dx%dx%d" % (name, os.getpid(), W, H, F))
            names = ["%s_%04d.jpg" % (stem, i) for i in range(F)]
            try:
                for i in range(F if args.jpeg_writer == "pillow" else 0):
                    fr = clip[i]
                    Image.fromarray(np.stack([(fr >> 16) & 255, (fr >> 8) & 255, fr & 255], -1).astype(np.uint8), "RGB").save(names[i], "JPEG", quality=90, subsampling=2, **opts)
                for i in range(0, F if args.jpeg_writer == "library" else 0, 16):
                    import torch
                    from tiler_amd import stages
                    dev = torch.from_numpy(np.ascontiguousarray(clip[i:i + 16]).view(np.int32)).cuda()
                    for k, data in enumerate(stages.jpeg_encode(dev, 90, "420", opts.get("restart_marker_rows", 0))):
                        with open(names[i + k], "wb") as fh:
                            fh.write(data)
                leg = dict(file_bytes=sum(os.path.getsize(n) for n in names), writer=args.jpeg_writer)
                encs, ms, info = {}, {"device": [], "host": []}, None
                for where in ms:
                    encs[where] = TilingEncoder()
                    encs[where].LoadDefaultSettings()
                    encs[where].InputFileName = stem + "_%.4d.jpg"
                for p in range(args.passes + 1):
                    for where in ms:  # alternating, so that a drift of the machine falls on both
                        os.environ["TM_JPEG_DECODE"] = where
                        t0 = time.perf_counter()
                        info = encs[where].OpenInput()
                        encs[where].Run(S.esLoad)
                        ms[where].append((time.perf_counter() - t0) * 1e3)
                for where in ms:
                    leg[where] = dict(stats(ms[where][1:]), video=info, input_stats=encs[where].InputStats())
                    encs[where].close()
                out["load_jpeg_" + name] = leg
            finally:
                os.environ.pop("TM_JPEG_DECODE", None)
                for n in names:
                    if os.path.exists(n):
                        os.remove(n)

    if args.mode == "gif":
        from PIL import Image
        rgb = lambda fr: np.stack([(fr >> 16) & 255, (fr >> 8) & 255, fr & 255], -1).astype(np.uint8)  # noqa: E731
        yy, xx = np.mgrid[0:H, 0:W]
        cartoon = []
        for i in range(F):  # plain areas and a few shapes that move: what a screen capture or a sprite sheet looks like
            fr = np.where(yy < H // 2, 0x88CCEE, 0x55AA55).astype(np.int64)
            for k in range(6):
                cx, cy, r = (37 * k + (3 + k) * i) % W, (53 * k + (2 + k) * i) % H, 12 + 5 * k
                fr[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] = (0xFF4040, 0xFFE040, 0x4040FF, 0xFFFFFF, 0x202020, 0xFF80C0)[k]
            cartoon.append(fr)
        for name, frames in (("bench_256", [clip[i] for i in range(F)]), ("cartoon_16", cartoon)):
            path = os.path.join(args.dir, "time_gif_load_%s_%d_%dx%dx%d.gif" % (name, os.getpid(), W, H, F))
            try:
                ims = [Image.fromarray(rgb(fr), "RGB").quantize(256 if name == "bench_256" else 16, dither=Image.Dither.NONE) for fr in frames]
                ims[0].save(path, "GIF", save_all=True, append_images=ims[1:], duration=40, loop=0)
                leg = dict(file_bytes=os.path.getsize(path))
                encs, ms, info = {}, {"device": [], "host": []}, None
                for where in ms:
                    encs[where] = TilingEncoder()
                    encs[where].LoadDefaultSettings()
                    encs[where].InputFileName = path
                for p in range(args.passes + 1):
                    for where in ms:  # alternating, so that a drift of the machine falls on both
                        os.environ["TM_GIF_DECODE"] = where
                        t0 = time.perf_counter()
                        info = encs[where].OpenInput()
                        encs[where].Run(S.esLoad)
                        ms[where].append((time.perf_counter() - t0) * 1e3)
                same = None
                for where in ms:
                    leg[where] = dict(stats(ms[where][1:]), video=info, input_stats=encs[where].InputStats())
                    got = encs[where].RenderFrames(input=True, device=False)
                    leg["same_frames"] = True if same is None else bool(np.array_equal(got, same))
                    same = got
                    encs[where].close()
                out["load_gif_" + name] = leg
            finally:
                os.environ.pop("TM_GIF_DECODE", None)
                if os.path.exists(path):
                    os.remove(path)

    if args.mode in ("file", "both", "all"):
        path = os.path.join(args.dir, "time_file_load_%d.y4m" % os.getpid())
        try:
            with open(path, "wb") as f:
                f.write(b"YUV4MPEG2 W%d H%d F24:1 Ip A1:1 C420jpeg\n" % (W, H))
                for i in range(F):
                    y, u, v = rgb_to_yuv420(clip[i].astype(np.int64))
                    f.write(b"FRAME\n" + y.tobytes() + u.tobytes() + v.tobytes())
            enc = TilingEncoder()
            enc.LoadDefaultSettings()
            enc.InputFileName = path
            enc.Scaling = args.scaling
            ms, open_ms = [], []
            for p in range(args.passes + 1):
                t0 = time.perf_counter()
                info = enc.OpenInput()  # (a new probe: the Load behind it decodes the file again)
                t1 = time.perf_counter()
                enc.Run(S.esLoad)
                t2 = time.perf_counter()
                ms.append((t2 - t0) * 1e3)
                open_ms.append((t1 - t0) * 1e3)
            enc.close()
            out["load_file_y4m420"] = dict(stats(ms[1:]), open_input_median_ms=statistics.median(open_ms[1:]), video=info)
        finally:
            if os.path.exists(path):
                os.remove(path)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
