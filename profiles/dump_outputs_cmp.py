"""Compare two `bench.py --dump-outputs` directories entry by entry (the r06 / r08 `*_dump_outputs_cmp.txt` tables).
usage: python profiles/dump_outputs_cmp.py DIR_A DIR_B [names.txt]   (names.txt: one parameter name per line, in grad_norm order)"""
import os
import sys

import numpy as np

a_dir, b_dir = sys.argv[1], sys.argv[2]
names = open(sys.argv[3]).read().split() if len(sys.argv) > 3 and os.path.exists(sys.argv[3]) else None
for f in sorted(os.listdir(a_dir)):
    if not f.endswith(".npy"):
        continue
    a, b = np.load(os.path.join(a_dir, f)).ravel(), np.load(os.path.join(b_dir, f)).ravel()
    assert a.shape == b.shape, (f, a.shape, b.shape)
    diff = np.flatnonzero(a.view(np.uint32 if a.dtype == np.float32 else np.uint64) != b.view(np.uint32 if b.dtype == np.float32 else np.uint64))
    key = f[:-4]
    if diff.size == 0:
        print(f"{key}: bit-identical ({a.size} entries)")
        continue
    rel = np.abs(a[diff].astype(np.float64) - b[diff]) / np.maximum(np.abs(a[diff].astype(np.float64)), 1e-300)
    print(f"{key}: {diff.size} of {a.size} entries differ, max rel {rel.max():.3e}")
    if diff.size <= 64:
        print(f"  parameter indices: {diff.tolist()}")
        if names and key == "grad_norm":
            print(f"  names: {[names[i] for i in diff]}")
        print(f"  rel: {[f'{r:.2e}' for r in rel]}")
