"""Generate tests/golden/online_pool_known.npz: what the REFERENCE's online hard mining keeps and replays on known key streams.

The reference's own statements are ast-extracted from its source text at run time and run here in a temporary directory:
``save_data_online`` / ``save_data_online3`` (train.py) and the ``__init__`` of ``OnlineHMData`` / ``OnlineHMData3`` (data.py,
with ``Dataset = object``).  The batches are 2x2x2 arrays whose first element is a sample id (id = call * B + i), handed over
behind a stand-in for the three tensor methods the functions call.  Only data is written: the keys of every call, the ids that
survive after every call, and the ids ``OnlineHMData`` selects for several rates.

Condition on the inputs: all keys of a run are DISTINCT float32 values (a seeded permutation of k / 1024), formatted like
train.py:446 does (``str(tensor.item())``).  The reference is only well defined without ties: equal keys of one iteration
share a file name and overwrite each other, equal keys of different iterations are evicted in ``os.listdir`` order.

Usage: python scripts/make_golden_online_pool.py --reference PATH_TO_REFERENCE_CHECKOUT
"""
import argparse
import ast
import bisect
import os
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "online_pool_known.npz")
CALLS = 40
RUNS = [(fn, B, limits) for fn in ("save_data_online", "save_data_online3") for B in (3, 4) for limits in (1, 7, 10)]
RATES = (1.0, 0.33, 0.5, 0.05, 0.9)          # int(0.05 * n) == 0 for every n <= 10: the slice that selects everything


class Batch:
    """Stand-in for a tensor: save_data_online calls .detach().cpu().numpy() and nothing else."""

    def __init__(self, a):
        self.a = a
        self.shape = a.shape

    def detach(self):
        return self

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def extract(path, names, namespace):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), os.path.basename(path), "exec"), namespace)


def extract_inits(path, names, namespace):
    """{class name: its __init__ as a plain function}."""
    tree = ast.parse(open(path).read())
    out = {}
    for cls in [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in names]:
        init = next(m for m in cls.body if isinstance(m, ast.FunctionDef) and m.name == "__init__")
        ns = dict(namespace)
        exec(compile(ast.Module(body=[init], type_ignores=[]), os.path.basename(path), "exec"), ns)
        out[cls.name] = ns["__init__"]
    return out


def ids_in(folder, sub):
    return sorted(int(np.load(os.path.join(folder, sub, n)).reshape(-1)[0]) for n in os.listdir(os.path.join(folder, sub)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (train.py, data.py)")
    ref = ap.parse_args().reference
    ns = {"os": os, "np": np, "bisect": bisect}
    extract(os.path.join(ref, "train.py"), ("save_data_online", "save_data_online3"), ns)
    inits = extract_inits(os.path.join(ref, "data.py"), ("OnlineHMData", "OnlineHMData3"), {"os": os, "Dataset": object})
    rng = np.random.default_rng(20261018)
    data = {"nrun": np.array(len(RUNS)), "rates": np.array(RATES, np.float64)}
    for r, (fn, B, limits) in enumerate(RUNS):
        three = fn.endswith("3")
        keys = (rng.permutation(CALLS * B).astype(np.float32) / np.float32(1024)).reshape(CALLS, B)
        assert len(set(keys.reshape(-1).tolist())) == CALLS * B
        survivors = np.full((CALLS, limits), -1, np.int64)
        with tempfile.TemporaryDirectory() as tmp:
            subs = ("image", "label", "weight") + (("skel",) if three else ())
            for sub in subs:
                os.mkdir(os.path.join(tmp, sub))
            for it in range(CALLS):
                ids = np.arange(it * B, (it + 1) * B)
                arrs = []
                for sub in subs:
                    a = np.zeros((B, 2, 2, 2), np.float32)
                    a[:, 0, 0, 0] = ids % 100 if sub in ("label", "skel") else ids        # (label / skel are cast to int8)
                    arrs.append(Batch(a))
                names = [str(torch.tensor(k).item()) + "_" + str(it) + ".npy" for k in keys[it]]
                ns[fn](tmp, *arrs, names, limits=limits)
                alive = ids_in(tmp, "image")
                assert len(alive) == min(limits, (it + 1) * B), (fn, B, limits, it, alive)
                for sub in subs[1:]:
                    assert sorted(os.listdir(os.path.join(tmp, sub))) == sorted(os.listdir(os.path.join(tmp, "image")))
                survivors[it, :len(alive)] = alive
            for k, rate in enumerate(RATES):
                self = types.SimpleNamespace()
                inits["OnlineHMData3" if three else "OnlineHMData"](self, tmp, 8, rate=rate)
                picked = [int(np.load(os.path.join(tmp, "image", n)).reshape(-1)[0]) for n in self.name_list]
                data[f"run{r}_replay{k}"] = np.array(picked, np.int64)
        data[f"run{r}_keys"] = keys
        data[f"run{r}_survivors"] = survivors
        data[f"run{r}_config"] = np.array([int(three), B, limits], np.int64)
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
