"""A video file to a .gtm: python tools/encode_file.py IN OUT.gtm [--scaling S --start N --frames N --yuv auto|bt601|bt601-full|tiler|bt709|bt709-full]
                                                               [--raw-rgb LAYOUT --size WxH --fps F [--depth D]] [--pngs]
                                                               [--png-decode host|device] [--jpeg-decode host|device]
                                                               [--gif-decode host|device] [--gif-background RRGGBB]

IN is a Y4M file (`ffmpeg -i clip.mp4 -f yuv4mpegpipe clip.y4m`), an animated GIF (every image a frame, at the file's rate; --scaling must stay 1), a .gtm stream (its frames are played on the device and encoded again;
--scaling must stay 1) or a Format pattern naming a PNG or baseline JPEG sequence (frame_%.4d.png, frame_%.4d.jpg; key frames where a frame_NNNN.kf file exists).
With --raw-rgb IN is a headerless file of RGB frames such as `ffmpeg -i clip.mp4 -f rawvideo -pix_fmt rgb24 clip.rgb` writes (LAYOUT: rgb24,
bgr24, rgba, bgra, argb, abgr, rgb48, bgr48, rgba64, bgra64, rgbp, gbrp, gray; --depth D > 8: rgbp / gbrp / gray hold little-endian words of
D bits, as gbrp10le does): it is mapped, not read, and lent to the encoder as it lies (SetFramesRGB), so --scaling applies, and --start and
--frames slice the mapping.  --pngs: the decoded frames are also written as OUT_NNNN.png beside the stream, coded on the device
(GeneratePNGs at level 1).  --png-decode: where a PNG sequence is decoded (SetPngDecode; the default is the library's).  Prints the video as Load found it and the FrameQuality of the encode."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tiler_amd import rgb_in  # noqa: E402
from tiler_amd.encoder import TilingEncoder, TInputYUV  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("input")
ap.add_argument("output")
ap.add_argument("--scaling", type=float, default=1.0)
ap.add_argument("--start", type=int, default=0)
ap.add_argument("--frames", type=int, default=0)
YUV = ["auto", "bt601", "bt601-full", "tiler", "bt709", "bt709-full"]  # (the index is TInputYUV)
ap.add_argument("--yuv", choices=YUV, default="auto")
ap.add_argument("--raw-rgb", choices=sorted(rgb_in.LAYOUTS), default=None)
ap.add_argument("--size", default=None, help="WxH of a --raw-rgb file's frames")
ap.add_argument("--fps", type=float, default=None, help="frame rate of a --raw-rgb file")
ap.add_argument("--depth", type=int, default=None, help="bits per sample of a --raw-rgb file's 16-bit words")
ap.add_argument("--pngs", action="store_true", help="also write the decoded frames as OUT_NNNN.png (deflate on the device)")
ap.add_argument("--png-decode", choices=["host", "device"], default=None, help="where a PNG sequence is decoded")
ap.add_argument("--jpeg-decode", choices=["host", "device"], default=None, help="where a JPEG sequence (frame_%%.4d.jpg) is decoded")
ap.add_argument("--gif-decode", choices=["host", "device"], default=None, help="where an animated GIF is decoded")
ap.add_argument("--gif-background", default=None, help="the canvas colour of a GIF, RRGGBB in hex (default: the file's background colour)")
args = ap.parse_args()
enc = TilingEncoder()
enc.LoadDefaultSettings()
enc.OutputFileName = args.output
enc.Scaling = args.scaling
if args.png_decode:
    enc.SetPngDecode(args.png_decode)
if args.jpeg_decode:
    enc.SetJpegDecode(args.jpeg_decode)
if args.gif_decode:
    enc.SetGifDecode(args.gif_decode)
if args.gif_background:
    enc.SetGifBackground(int(args.gif_background, 16))
if args.raw_rgb:
    import numpy as np
    if not args.size or not args.fps:
        ap.error("--raw-rgb needs --size WxH and --fps F")
    w, h = (int(v) for v in args.size.lower().split("x"))
    kind, nch, _, item = rgb_in.LAYOUTS[args.raw_rgb]
    item = item or (2 if (args.depth or 8) > 8 else 1)
    shape = {"packed": (h, w, nch), "planar": (3, h, w), "gray": (h, w)}[kind]
    raw = np.memmap(args.input, np.uint8 if item == 1 else np.dtype("<u2"), "r")
    total = raw.size // int(np.prod(shape))  # (a last frame cut short does not count)
    clip = raw[:total * int(np.prod(shape))].reshape((total,) + shape)
    clip = clip[args.start:args.start + args.frames] if args.frames > 0 else clip[args.start:]
    if len(clip) < max(args.frames, 1):
        sys.exit("%s holds %d whole frames of %dx%d %s: frames [%d,+%d) are not all there" % (args.input, total, w, h, args.raw_rgb, args.start, max(args.frames, 1)))
    enc.SetFramesRGB(clip, args.raw_rgb, fps=args.fps, depth=args.depth)
else:
    enc.InputFileName, enc.StartFrame, enc.FrameCount = args.input, args.start, args.frames
    enc.InputYUV = TInputYUV(YUV.index(args.yuv))
enc.Run()  # Load opens the input by itself (or reads the lent clip); Save follows Reindex because OutputFileName is set
if args.pngs:
    enc.SetPngOptions(level=1)
    enc.GeneratePNGs()
q = enc.FrameQuality()
print(json.dumps(dict(video=enc.VideoInfo(), keyframes=enc.KeyFrames().tolist(), tiles=enc.counts()["tiles"], clip_psnr=q["clip_psnr"],
                      clip_ssim_y=q["clip_ssim_y"], psnr=[round(float(v), 3) for v in q["psnr"]])))
enc.close()
