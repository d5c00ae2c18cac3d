"""Fréchet Inception Distance between two sets of images, or between saved statistics.

    python tools/fid_npy.py A B [--ckpt inception.pth] [--batch 16] [--quant pil|np] [--save-a a.npz] [--save-b b.npz]
                            [--isc] [--kid] [--prc] [--save-feats-a fa.npz] [--save-feats-b fb.npz]

A and B are each either an .npy image stack -- uint8 [N, H, W, 3] (what `bench.py --dump-outputs DIR` writes) or float32 [N, 3, H, W] in
[-1, 1] -- or an .npz of statistics (mu, sigma, n) written by --save-a / --save-b or FeatureStatistics.save: precomputed reference
statistics are how the distance is used in practice.  Prints one line with the distance.

--isc adds one line per side with the Inception Score (mean and std over --isc-splits splits), --kid one line with the Kernel
Inception Distance between the sides (mean and std over --kid-subsets subsets of --kid-subset-size); both are
frido_amd.fidelity's, whose docstrings are their specification.  They need per-sample rows, which statistics files do not hold: for
them A and B are image stacks or saved BANKS, an .npz with `features` [n, 2048] (--save-feats-a / --save-feats-b write them; a bank
[n, 1008] is taken as logits and serves --isc alone).  A side given as a bank takes part in the distance line through its rows.

--prc adds one line with improved precision and recall and density and coverage at the neighbourhood --prc-k
(frido_amd.manifold.prdc, whose docstring is the specification).  Side B is the REAL one, as `fidelity --input1 PRED --input2 GT` has
it; like --kid it wants features on both sides.

--ckpt is a LOCAL state_dict of the published FID Inception weights (pt_inception-2015-12-05); nothing is downloaded.  WITHOUT it the
extractor holds torch's initialisation and the printed number measures nothing about image quality; the tool says so."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def statistics_of(path, extractor, batch, quant, want_feats=False, want_logits=False):
    """(the side's FeatureStatistics, its bank of features, its bank of logits); a bank is None where it was not asked for or the
    file cannot give it (a bank of logits holds neither statistics nor features)."""
    from frido_amd import fid, fidelity, pipeline
    banks = want_feats or want_logits
    if banks and not torch.cuda.is_available():
        sys.exit("tools/fid_npy.py: --isc, --kid and saved banks need the HIP device (saved statistics do not); there is no CPU path")
    if path.endswith(".npz") and "features" in np.load(path).files:
        if not torch.cuda.is_available():
            sys.exit("tools/fid_npy.py: saved banks need the HIP device (saved statistics do not); there is no CPU path")
        bank = fidelity.FeatureBank.load(path, "cuda")
        if bank.D == fidelity.LOGITS:
            return None, None, bank
        lb = fidelity.FeatureBank(fidelity.LOGITS, "cuda").append(extractor().logits(bank.rows())) if want_logits else None
        return fid.FeatureStatistics(bank.D, "cuda").update(bank.rows()), bank, lb
    if path.endswith(".npz"):
        if banks:
            sys.exit(f"tools/fid_npy.py: {path} holds statistics (mu, sigma, n); --isc and --kid need an image stack or a saved bank")
        return fid.FeatureStatistics.load(path), None, None
    arr = np.load(path, mmap_mode="r")
    if not ((arr.dtype == np.uint8 and arr.ndim == 4 and arr.shape[3] == 3) or (arr.dtype == np.float32 and arr.ndim == 4 and arr.shape[1] == 3)):
        sys.exit(f"tools/fid_npy.py: {path} holds {arr.dtype} {arr.shape}; expected uint8 [N, H, W, 3] or float32 [N, 3, H, W]")
    ex = extractor()
    ex.quant = quant
    st = None
    fb = fidelity.FeatureBank(fid.FEATURES, "cuda") if want_feats else None
    lb = fidelity.FeatureBank(fidelity.LOGITS, "cuda") if want_logits else None
    for i in range(0, arr.shape[0], batch):
        x = torch.from_numpy(np.ascontiguousarray(arr[i:i + batch])).cuda()
        if banks:
            st = pipeline.fidelity_features(ex, x, stats=st or fid.FeatureStatistics(fid.FEATURES, "cuda"), feats=fb, logits=lb)[0]
        else:
            st = pipeline.fid_statistics(ex, x, st)
    return st, fb, lb


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--ckpt", default=None, help="local state_dict of the FID Inception weights")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--quant", default="pil", choices=["pil", "np"], help="8-bit quantisation of float images (uint8 stacks are taken as they are)")
    ap.add_argument("--save-a", default=None)
    ap.add_argument("--save-b", default=None)
    ap.add_argument("--isc", action="store_true", help="also print each side's Inception Score")
    ap.add_argument("--kid", action="store_true", help="also print the Kernel Inception Distance between the sides")
    ap.add_argument("--prc", action="store_true", help="also print precision / recall and density / coverage of side A against the real side B")
    ap.add_argument("--prc-k", type=int, default=3, help="the neighbourhood of --prc")
    ap.add_argument("--isc-splits", type=int, default=10)
    ap.add_argument("--kid-subsets", type=int, default=100)
    ap.add_argument("--kid-subset-size", type=int, default=1000)
    ap.add_argument("--save-feats-a", default=None, help="write side A's features as a bank (.npz with `features`)")
    ap.add_argument("--save-feats-b", default=None)
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
    sides = {}
    for side, path, save in (("a", args.a, args.save_feats_a), ("b", args.b, args.save_feats_b)):
        sides[side] = statistics_of(path, extractor, args.batch, args.quant, want_feats=bool(args.kid or args.prc or save), want_logits=args.isc)
        if save:
            if sides[side][1] is None:
                sys.exit(f"tools/fid_npy.py: {path} gives no features to save")
            sides[side][1].save(save)
    sa, sb = sides["a"][0], sides["b"][0]
    if args.save_a and sa is not None:
        sa.save(args.save_a)
    if args.save_b and sb is not None:
        sb.save(args.save_b)
    note = "" if args.ckpt or "m" not in cache else "   (NO --ckpt: untrained extractor, the number measures nothing about image quality)"
    if sa is not None and sb is not None:
        if sa.D != sb.D:
            sys.exit(f"tools/fid_npy.py: the two sides have {sa.D} and {sb.D} features")
        d = pipeline.fid(sa, sb)
        print(f"frechet_distance {d:.6f}   n = {sa.n} / {sb.n}{note}")
    if args.isc:
        for side in ("a", "b"):
            lb = sides[side][2]
            mean, std = pipeline.inception_score(lb, splits=args.isc_splits)
            print(f"inception_score_{side} {mean:.6f} +- {std:.6f}   n = {lb.n}, splits = {args.isc_splits}{note}")
    if args.kid:
        fa, fb = sides["a"][1], sides["b"][1]
        if fa is None or fb is None:
            sys.exit("tools/fid_npy.py: --kid needs features on both sides; a bank of logits holds none")
        mean, std = pipeline.kid(fa, fb, subsets=args.kid_subsets, subset_size=args.kid_subset_size)
        print(f"kernel_inception_distance {mean:.6f} +- {std:.6f}   n = {fa.n} / {fb.n}, subsets = {args.kid_subsets} x {args.kid_subset_size}{note}")
    if args.prc:
        fa, fb = sides["a"][1], sides["b"][1]
        if fa is None or fb is None:
            sys.exit("tools/fid_npy.py: --prc needs features on both sides; a bank of logits holds none")
        r = pipeline.precision_recall(fb, fa, k=args.prc_k)
        print(f"precision_recall precision {r['precision']:.6f} recall {r['recall']:.6f} f_score {r['f_score']:.6f} density {r['density']:.6f} "
              f"coverage {r['coverage']:.6f}   n = {fa.n} / {fb.n}, k = {args.prc_k}{note}")


if __name__ == "__main__":
    main()
