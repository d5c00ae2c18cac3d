"""Fréchet Inception Distance between two sets of images, or between saved statistics.

    python tools/fid_npy.py A B [--ckpt inception.pth] [--batch 16] [--quant pil|np] [--save-a a.npz] [--save-b b.npz]

A and B are each either an .npy image stack -- uint8 [N, H, W, 3] (what `bench.py --dump-outputs DIR` writes) or float32 [N, 3, H, W] in
[-1, 1] -- or an .npz of statistics (mu, sigma, n) written by --save-a / --save-b or FeatureStatistics.save: precomputed reference
statistics are how the distance is used in practice.  Prints one line with the distance.

--ckpt is a LOCAL state_dict of the published FID Inception weights (pt_inception-2015-12-05); nothing is downloaded.  WITHOUT it the
extractor holds torch's initialisation and the printed number measures nothing about image quality; the tool says so."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def statistics_of(path, extractor, batch, quant):
    from frido_amd import fid, pipeline
    if path.endswith(".npz"):
        return fid.FeatureStatistics.load(path)
    arr = np.load(path, mmap_mode="r")
    if not ((arr.dtype == np.uint8 and arr.ndim == 4 and arr.shape[3] == 3) or (arr.dtype == np.float32 and arr.ndim == 4 and arr.shape[1] == 3)):
        sys.exit(f"tools/fid_npy.py: {path} holds {arr.dtype} {arr.shape}; expected uint8 [N, H, W, 3] or float32 [N, 3, H, W]")
    ex = extractor()
    ex.quant = quant
    st = None
    for i in range(0, arr.shape[0], batch):
        st = pipeline.fid_statistics(ex, torch.from_numpy(np.ascontiguousarray(arr[i:i + batch])).cuda(), st)
    return st


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--ckpt", default=None, help="local state_dict of the FID Inception weights")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--quant", default="pil", choices=["pil", "np"], help="8-bit quantisation of float images (uint8 stacks are taken as they are)")
    ap.add_argument("--save-a", default=None)
    ap.add_argument("--save-b", default=None)
    args = ap.parse_args()
    for p in (args.a, args.b):
        if not os.path.exists(p):
            sys.exit(f"tools/fid_npy.py: no such file: {p}")
    cache = {}

    def extractor():
        if "m" not in cache:
            if not torch.cuda.is_available():
                sys.exit("tools/fid_npy.py: image stacks need the HIP device (saved statistics do not); there is no CPU path")
            from frido_amd.models import FIDInceptionV3
            cache["m"] = FIDInceptionV3(ckpt=args.ckpt).cuda()
        return cache["m"]

    from frido_amd import pipeline
    sa = statistics_of(args.a, extractor, args.batch, args.quant)
    sb = statistics_of(args.b, extractor, args.batch, args.quant)
    if args.save_a:
        sa.save(args.save_a)
    if args.save_b:
        sb.save(args.save_b)
    if sa.D != sb.D:
        sys.exit(f"tools/fid_npy.py: the two sides have {sa.D} and {sb.D} features")
    d = pipeline.fid(sa, sb)
    note = "" if args.ckpt or "m" not in cache else "   (NO --ckpt: untrained extractor, the number measures nothing about image quality)"
    print(f"frechet_distance {d:.6f}   n = {sa.n} / {sb.n}{note}")


if __name__ == "__main__":
    main()
