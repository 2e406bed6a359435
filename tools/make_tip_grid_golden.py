"""Writes tests/golden/tip_grid_reference.npz: what the reference's own `eval_threshold`, `find_thresholds`
(code/main_custom.py), `cls_f1` and `cls_acc` (code/utils.py) return on small logits.  CPU only.

    python tools/make_tip_grid_golden.py --reference /path/to/the/reference/checkout

The four definitions are read from the reference tree when this runs (the function nodes are cut out of the two modules
and compiled on their own, so neither their imports nor their drivers run); this script holds none of their text.
`find_thresholds` is given fp32 logits widened to fp64 -- the contract of mmr_tip_adapter_grid -- and returns only the
best F1, so `eval_threshold` is wrapped to record every (threshold, f1, precision, recall) it is asked for: the
reference's threshold is the first recorded one whose F1 equals the F1 it returned (its update is a strict `>`), and
num_vals is the number of calls.  The counts stored next to it are taken at that threshold and checked here against the
reference's precision and recall bit for bit.
"""
import argparse
import ast
import os
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(60, 4, 0, 6.0), (41, 3, 1, 3.0), (25, 2, 2, 9.0), (90, 6, 3, 5.0)]        # rows, classes, seed, spread


def functions(path, names):
    with open(path) as f:
        tree = ast.parse(f.read())
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in nodes) == sorted(names), f"{path} does not define {names}"
    space = {"np": np, "torch": torch}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), space)
    return space


def make_logits(N, C, seed, spread):
    rng = np.random.RandomState(seed)
    labels = rng.randint(0, C, size=N)
    logits = 20.0 + spread * rng.randn(N, C) + 1.5 * spread * np.eye(C)[labels]
    return logits.astype(np.float32), labels.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (the directory that holds code/)")
    args = ap.parse_args()
    main_custom = functions(os.path.join(args.reference, "code", "main_custom.py"), ["eval_threshold", "find_thresholds"])
    utils = functions(os.path.join(args.reference, "code", "utils.py"), ["cls_f1", "cls_acc"])
    ref_eval = main_custom["eval_threshold"]
    calls = []

    def recording_eval(pos_res, neg_res, threshold):
        out = ref_eval(pos_res, neg_res, threshold)
        calls.append((float(threshold),) + tuple(float(v) for v in out))
        return out

    main_custom["eval_threshold"] = recording_eval
    out = {"cases": np.array(CASES, dtype=np.float64)}
    warnings.simplefilter("ignore")
    for k, (N, C, seed, spread) in enumerate(CASES):
        logits, labels = make_logits(N, C, seed, spread)
        wide = logits.astype(np.float64)
        rows = []
        for c in range(C):
            pos, neg = wide[labels == c, c], wide[labels != c, c]
            calls.clear()
            with np.errstate(all="ignore"):
                f1 = float(main_custom["find_thresholds"](pos, neg, str(c), verbose=False))
            thr, tp, fp, fn = 0.0, 0, 0, 0
            if f1 > 0:
                thr, _, precision, recall = next(r for r in calls if r[1] == f1)
                tp, fp = int((pos >= thr).sum()), int((neg >= thr).sum())
                fn = len(pos) - tp
                assert tp / (tp + fp) == precision and tp / (tp + fn) == recall
            rows.append((f1, thr, tp, fp, fn, len(calls)))
        out[f"logits{k}"], out[f"labels{k}"] = logits, labels
        out[f"f1_{k}"] = np.array([r[0] for r in rows], dtype=np.float64)
        out[f"threshold{k}"] = np.array([r[1] for r in rows], dtype=np.float64)
        out[f"counts{k}"] = np.array([r[2:] for r in rows], dtype=np.int64)          # tp, fp, fn, num_vals
        t_logits, t_labels = torch.from_numpy(logits), torch.from_numpy(labels)
        out[f"cls{k}"] = np.array([utils["cls_f1"](t_logits, t_labels), utils["cls_acc"](t_logits, t_labels),
                                   utils["cls_acc"](t_logits, t_labels, exclude_class=C - 1)], dtype=np.float64)
    path = os.path.join(ROOT, "tests", "golden", "tip_grid_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
