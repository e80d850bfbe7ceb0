"""A video file to a .gtm: python tools/encode_file.py IN OUT.gtm [--scaling S --start N --frames N --yuv auto|bt601|bt601-full|tiler|bt709|bt709-full]

IN is a Y4M file (`ffmpeg -i clip.mp4 -f yuv4mpegpipe clip.y4m`), a .gtm stream (its frames are played on the device and encoded again;
--scaling must stay 1) or a Format pattern naming a PNG sequence (frame_%.4d.png; key frames where a frame_NNNN.kf file exists).  Prints the video as Load found it and the FrameQuality of the encode."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tiler_amd.encoder import TilingEncoder, TInputYUV  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("input")
ap.add_argument("output")
ap.add_argument("--scaling", type=float, default=1.0)
ap.add_argument("--start", type=int, default=0)
ap.add_argument("--frames", type=int, default=0)
YUV = ["auto", "bt601", "bt601-full", "tiler", "bt709", "bt709-full"]  # (the index is TInputYUV)
ap.add_argument("--yuv", choices=YUV, default="auto")
args = ap.parse_args()
enc = TilingEncoder()
enc.LoadDefaultSettings()
enc.InputFileName, enc.OutputFileName = args.input, args.output
enc.Scaling, enc.StartFrame, enc.FrameCount = args.scaling, args.start, args.frames
enc.InputYUV = TInputYUV(YUV.index(args.yuv))
enc.Run()  # Load opens the input by itself; Save follows Reindex because OutputFileName is set
q = enc.FrameQuality()
print(json.dumps(dict(video=enc.VideoInfo(), keyframes=enc.KeyFrames().tolist(), tiles=enc.counts()["tiles"], clip_psnr=q["clip_psnr"],
                      clip_ssim_y=q["clip_ssim_y"], psnr=[round(float(v), 3) for v in q["psnr"]])))
enc.close()
