"""Save alone on the bench clip:
  python tools/time_save.py --dir DIR [--reps 5] [--json OUT.json]            encodes the two clips of tools/time_player.py (1280 x 720 x 300,
                                                                              16 palettes, MotionPredictRadius 32 and 0) and times Save of each:
                                                                              wall clock around a call that ends synchronised, one warm-up Save
                                                                              first, then --reps Saves per configuration
  python tools/time_save.py --dir DIR --against parent [--rounds 3] ...       the same in child processes, this build and the library
                                                                              tiler_amd/lib/variants/libtilemotion_parent.so in turns
                                                                              (TM_LIB_VARIANT), so that the two are timed side by side
  python tools/time_save.py --dir DIR --only device|host|host1 --motion 0|1   one warm-up and one Save: the program to put behind
                                                                              `rocprofv3 --kernel-trace --stats --`
Configurations: "default" (no switch set), "device" (TM_SAVE_FINDER=device), "host" (TM_SAVE_FINDER=host), "host1" (TM_SAVE_FINDER=host
TM_HOST_THREADS=1: the one-thread writer of before).  A library without tm_get_save_stats (a build of an earlier commit) is timed under
"default" alone, wall time only.  Every configuration's file must be the same bytes."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, F = 1280, 720, 300
CONFIGS = {"default": {}, "device": {"TM_SAVE_FINDER": "device"}, "host": {"TM_SAVE_FINDER": "host"},
           "host1": {"TM_SAVE_FINDER": "host", "TM_HOST_THREADS": "1"}}
SWITCHES = ("TM_SAVE_FINDER", "TM_HOST_THREADS")


def encode(radius):
    import numpy as np
    import torch
    import bench
    from tiler_amd.encoder import TilingEncoder
    host = bench.synth_clip(np.empty((F, H, W), np.int32), freeze=False)
    enc = TilingEncoder()
    enc.LoadDefaultSettings()
    enc.PaletteCount, enc.PaletteSize = 16, 16
    enc.FrameTilingExtendedPaletteUsage = False
    enc.MotionPredictRadius = radius
    enc.SetVideo(W, H, 24.0, F)
    enc.SetFramesDevice(torch.from_numpy(host).cuda())
    enc.Run()
    return enc


def has_stats(enc):
    return hasattr(enc, "SaveStats") and getattr(enc._L, "tm_get_save_stats", None) is not None


def save_once(enc, path, env):
    import torch
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enc.Save(path)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    for k in SWITCHES:
        os.environ.pop(k, None)
    return wall, (enc.SaveStats() if has_stats(enc) else None)


def time_stream(radius, path, reps, only=None):
    enc = encode(radius)
    stats = has_stats(enc)
    names = [only] if only else (list(CONFIGS) if stats else ["default"])
    res, digest = dict(key_frames=len(enc.KeyFrames()), items=int(enc.counts()["frames"]) * enc.counts()["tm_w"] * enc.counts()["tm_h"], configs={}), None
    for name in names:
        save_once(enc, path, CONFIGS[name])  # warm-up: code objects, the pool, the page cache
        runs = [save_once(enc, path, CONFIGS[name]) for _ in range(max(reps, 1))]
        d = hashlib.sha256(open(path, "rb").read()).hexdigest()
        assert digest is None or d == digest, "Save under %s writes another file" % name
        digest = d
        c = dict(wall_ms=[r[0] for r in runs])
        if stats:
            last = runs[-1][1]
            c.update(finder=last["finder"], threads=last["threads"],
                     split_ms={k: statistics.median(r[1][k] for r in runs) for k in ("ms_commands", "ms_finder", "ms_parse", "ms_wall")})
            res["raw_bytes"], res["comp_bytes"] = last["raw_bytes"], last["comp_bytes"]
        res["configs"][name] = c
    res["file_bytes"], res["sha256"] = os.path.getsize(path), digest
    enc.close()
    return res


def child(args):
    out = dict(lib=os.environ.get("TM_LIB_VARIANT", ""), reps=args.reps, streams={})
    for motion, radius in ((1, 32), (0, 0)):
        if args.only and motion != args.motion:
            continue
        out["streams"]["motion32" if motion else "motion0"] = time_stream(radius, os.path.join(args.dir, "save_motion%d.gtm" % radius), 1 if args.only else args.reps, args.only)
    return out


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json")
    ap.add_argument("--against", help="a library variant (tiler_amd/lib/variants/libtilemotion_<name>.so) to time in turns with this build")
    ap.add_argument("--only", choices=list(CONFIGS))
    ap.add_argument("--motion", type=int, default=1)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    if args.child or not args.against:
        result = child(args)
        if not args.child:
            for s in result["streams"].values():
                for c in s["configs"].values():
                    c["wall_ms"] = spread(c["wall_ms"])
    else:
        # this build and the other library in turns, a fresh process each time (a process loads one library)
        runs = {"": [], args.against: []}
        for _ in range(args.rounds):
            for lib in ("", args.against):
                env = dict(os.environ)
                env.pop("TM_LIB_VARIANT", None)
                if lib:
                    env["TM_LIB_VARIANT"] = lib
                tmp = os.path.join(args.dir, "child.json")
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--dir", args.dir, "--reps", str(args.reps), "--json", tmp, "--child"], env=env,
                                      timeout=600)
                runs[lib].append(json.load(open(tmp)))
        result = dict(clip="%d x %d x %d, bench.synth_clip, 16 palettes of 16" % (W, H, F), reps=args.reps, rounds=args.rounds, streams={})
        for stream in ("motion32", "motion0"):
            first = runs[""][0]["streams"][stream]
            res = {k: first[k] for k in ("key_frames", "items", "raw_bytes", "comp_bytes", "file_bytes", "sha256") if k in first}
            assert all(r["streams"][stream]["sha256"] == first["sha256"] for lib in runs for r in runs[lib]), "the two libraries write different files"
            res["this_build"] = {}
            for name in first["configs"]:
                walls = [w for r in runs[""] for w in r["streams"][stream]["configs"][name]["wall_ms"]]
                c = dict(wall_ms=spread(walls), per_round_median=[statistics.median(r["streams"][stream]["configs"][name]["wall_ms"]) for r in runs[""]])
                for k in ("finder", "threads", "split_ms"):
                    c[k] = first["configs"][name].get(k)
                res["this_build"][name] = c
            pw = [[w for w in r["streams"][stream]["configs"]["default"]["wall_ms"]] for r in runs[args.against]]
            res[args.against] = dict(wall_ms=spread([w for r in pw for w in r]), per_round_median=[statistics.median(r) for r in pw])
            result["streams"][stream] = res
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
