"""Fixtures tests/golden/mixup_*.npz: seeded runs of the REFERENCE's Mixup (timm1/data/mixup.py, loaded from the reference checkout by file path;
it imports only numpy and torch) on CPU tensors.

    python tests/golden/make_mixup_golden.py [--reference /path/to/checkout]

Per configuration: the constructor arguments (``cfg``, a dict literal), the seed, the input ``x0`` (6, 3, 7, 9) float32 and the labels (K = 11), and for
FOUR consecutive calls from one seeded ``np.random`` stream -- each on a fresh copy of x0 -- the mixed batch ``x_<c>`` and the target ``t_<c>``; then
``tail``, one ``np.random.rand()`` drawn after the fourth call, which pins the stream position.  Only these arrays are stored.

Seeds are searched so that the fixtures cover what they are for (asserted below): the four calls of the recipes' batch configuration hold both a mixup
call and a CutMix call, and the prob = 0.5 configuration holds both touched and untouched images.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N, C, H, W, K, CALLS = 6, 3, 7, 9, 11, 4
RECIPE = dict(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=K)     # --mixup 0.8 --cutmix 1.0 --smoothing 0.1
CONFIGS = {
    "batch_recipe": dict(RECIPE, mode="batch"),
    "batch_mixup_only": dict(mixup_alpha=0.8, cutmix_alpha=0.0, label_smoothing=0.1, num_classes=K, mode="batch"),
    "batch_cutmix_only": dict(mixup_alpha=0.0, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=K, mode="batch"),
    "batch_minmax": dict(RECIPE, cutmix_minmax=(0.2, 0.8), mode="batch"),
    "batch_no_correct_lam": dict(RECIPE, correct_lam=False, mode="batch"),
    "batch_prob0": dict(RECIPE, prob=0.0, mode="batch"),
    "pair_recipe": dict(RECIPE, mode="pair"),
    "elem_recipe": dict(RECIPE, mode="elem"),
    "elem_prob05": dict(RECIPE, prob=0.5, mode="elem"),
}


def load_reference(checkout):
    path = os.path.join(checkout, "timm1", "data", "mixup.py")
    spec = importlib.util.spec_from_file_location("reference_timm_data_mixup", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(N, C, H, W, generator=g)
    labels = torch.randint(0, K, (N,), generator=g)
    return x0, labels


def run(ref, cfg, seed):
    """The four calls, plus what the parameter draws said (for the coverage assertions)."""
    x0, labels = inputs(seed)
    fn = ref.Mixup(**cfg)
    seen = {"cutmix": [], "lam": []}
    per_batch, per_elem = fn._params_per_batch, fn._params_per_elem

    def spy_batch():
        lam, cut = per_batch()
        seen["cutmix"].append(bool(cut) and lam != 1.); seen["lam"].append(np.array([lam]))
        return lam, cut

    def spy_elem(n):
        lam, cut = per_elem(n)
        seen["cutmix"].append(bool(np.any(cut & (lam != 1.)))); seen["lam"].append(lam.copy())
        return lam, cut
    fn._params_per_batch, fn._params_per_elem = spy_batch, spy_elem
    np.random.seed(seed)
    out = {"cfg": np.array(repr(cfg)), "seed": np.array(seed), "x0": x0.numpy().copy(), "labels": labels.numpy().copy()}
    for c in range(CALLS):
        x = x0.clone()
        got_x, got_t = fn(x, labels)
        assert got_x is x and got_t.dtype == torch.float32 and got_t.shape == (N, K)
        out["x_%d" % c], out["t_%d" % c] = x.numpy().copy(), got_t.numpy().copy()
    out["tail"] = np.array(np.random.rand())
    return out, seen


def covers(name, seen):
    lam = np.concatenate(seen["lam"])
    if name == "batch_recipe":                                   # a mixup call and a CutMix call
        return any(seen["cutmix"]) and not all(seen["cutmix"]) and bool(np.all(lam != 1.))
    if name == "elem_prob05":                                    # touched and untouched images in every call
        return all(bool(np.any(l == 1.)) and bool(np.any(l != 1.)) for l in seen["lam"]) and any(seen["cutmix"])
    if name == "batch_prob0":
        return bool(np.all(lam == 1.))
    if name in ("pair_recipe", "elem_recipe"):                   # both kinds among the images
        return any(seen["cutmix"]) and bool(np.all(lam != 1.))
    return True


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import ref_modules
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=ref_modules.REF)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    total = 0
    for i, (name, cfg) in enumerate(CONFIGS.items()):
        for seed in range(100 * (i + 1), 100 * (i + 1) + 50):
            out, seen = run(ref, cfg, seed)
            if covers(name, seen):
                break
        else:
            raise SystemExit("no seed covers " + name)
        assert covers(name, seen)
        path = os.path.join(HERE, "mixup_%s.npz" % name)
        np.savez_compressed(path, **out)
        total += os.path.getsize(path)
        print("%-22s seed %d  %d bytes  cutmix calls %s" % (name, seed, os.path.getsize(path), seen["cutmix"]))
    print("total %d bytes" % total)


if __name__ == "__main__":
    main()
