"""Writes tests/golden/index_kmeans_sklearn.npz: the clustering quality the reference's own reducer reaches on one seeded data
set, for tests/test_index_build_gpu.py to hold rvc_amd.lib.kmeans.lloyd against.  Run once on a CPU box with scikit-learn; the
GPU test reads only the file.

The reducer is extract_index.py:46-55's call -- MiniBatchKMeans(n_clusters=10000, batch_size=256 * cpu_count(),
compute_labels=False, init="random") -- with the hard-coded cluster count replaced (128), the batch size pinned to that of an
8-core host (2048) and a seed added (0..4).  Stored: the recipe arguments, the float64 sum of the data (so the test knows it
regenerated the same matrix) and the five full-data inertias, each the float64 sum over rows of the squared distance to the
nearest fitted centre."""
import os
import sys

import numpy as np

RECIPE = (0, 20480, 256, 512, 0.05)   # clustered(seed, n, d, n_centres, jitter)
K = 128
SEEDS = (0, 1, 2, 3, 4)


def clustered(seed, n, d, n_centres, jitter):
    r = np.random.default_rng(seed)
    c = r.standard_normal((n_centres, d)).astype(np.float32) * 0.3
    return (c[r.integers(0, n_centres, n)] + r.standard_normal((n, d)).astype(np.float32) * jitter).astype(np.float32)


def inertia64(x, centres):
    x64, c64 = x.astype(np.float64), np.asarray(centres, dtype=np.float64)
    d2 = (x64 ** 2).sum(1)[:, None] - 2.0 * x64 @ c64.T + (c64 ** 2).sum(1)[None, :]
    best = d2.argmin(1)
    return float(((x64 - c64[best]) ** 2).sum())


def main():
    from sklearn.cluster import MiniBatchKMeans
    import sklearn
    x = clustered(*RECIPE)
    inertias = []
    for s in SEEDS:
        km = MiniBatchKMeans(n_clusters=K, batch_size=2048, compute_labels=False, init="random", random_state=s).fit(x)
        inertias.append(inertia64(x, km.cluster_centers_))
        print(f"seed {s}: inertia {inertias[-1]:.6f}")
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "index_kmeans_sklearn.npz")
    np.savez(out, recipe=np.array(RECIPE, dtype=np.float64), k=np.int64(K), seeds=np.array(SEEDS, dtype=np.int64),
             data_sum=np.float64(x.astype(np.float64).sum()), inertias=np.array(inertias, dtype=np.float64),
             sklearn_version=np.array(sklearn.__version__))
    print("wrote", out)


if __name__ == "__main__":
    sys.exit(main())
