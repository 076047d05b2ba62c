"""Build the retrieval index of an experiment: ``<exp_dir>/extracted/*.npy`` -> ``<exp_dir>/<basename>.index``.

This is the reference's rvc/train/process/extract_index.py step by step -- concatenate the extracted features in sorted file
order, shuffle, reduce to k-means centres above 2e5 rows (``Auto`` / ``KMeans``), ``n_ivf = min(16 sqrt(N), N // 39)``, an
``IVF{n_ivf},Flat`` index with ``nprobe = 1``, write it -- with the clustering on the device (rvc_amd.lib.kmeans, K16) and the
file written by rvc_amd.lib.faiss_index instead of faiss and scikit-learn on the CPU.

    python -m rvc_amd.train.process.extract_index EXP_DIR Auto
"""
from __future__ import annotations

import os
import sys

import numpy as np

from rvc_amd.lib import faiss_index, kmeans

ALGORITHMS = ("Auto", "Faiss", "KMeans")
INDEX_DIMS = (256, 512, 768, 1024)   # what the IVF search accepts (rvc_knn_rank_candidates)


def n_ivf(n_rows: int) -> int:
    """extract_index.py:59."""
    return min(int(16 * np.sqrt(n_rows)), n_rows // 39)


def _missing_message(feature_dir: str) -> str:
    return (f"Feature to generate index file not found at {feature_dir}. Did you run preprocessing and feature extraction steps?")


def extract_index(exp_dir, index_algorithm="Auto", *, device="cuda:0", seed=None, kmeans_threshold=200_000,
                  kmeans_clusters=10_000, kmeans_iterations=20):
    """-> the path of ``<exp_dir>/<basename>.index`` (written now, or found already there), or ``None`` when ``extracted/`` is
    missing or the build failed; both are reported on stdout in the reference's words, and no exception leaves this function.

    ``seed``: of the shuffle and of both k-means initialisations; ``None`` draws fresh entropy, as the reference's unseeded
    ``np.random.shuffle`` does.  ``kmeans_*``: the reference's hard-coded 2e5 rows / 10000 clusters, and the iteration count of
    the reduction (the reference runs mini-batch updates until scikit-learn's own stopping rule; here a fixed count)."""
    exp_dir = str(exp_dir)
    index_algorithm = str(index_algorithm)
    try:
        feature_dir = os.path.join(exp_dir, "extracted")
        model_name = os.path.basename(exp_dir)
        if not os.path.exists(feature_dir):
            print(_missing_message(feature_dir))
            return None
        index_filepath = os.path.join(exp_dir, f"{model_name}.index")
        if os.path.exists(index_filepath):
            return index_filepath
        npys = [np.load(os.path.join(feature_dir, name)) for name in sorted(os.listdir(feature_dir))]
        big_npy = np.concatenate(npys, axis=0)
        if big_npy.ndim != 2 or big_npy.shape[1] not in INDEX_DIMS:
            raise ValueError(f"extracted features must be [rows, d] with d in {INDEX_DIMS}, got {big_npy.shape}")
        big_npy = np.ascontiguousarray(big_npy, dtype=np.float32)
        rng = np.random.default_rng(seed)
        big_npy = big_npy[rng.permutation(big_npy.shape[0])]

        if big_npy.shape[0] > kmeans_threshold and index_algorithm in ("Auto", "KMeans"):
            import torch
            centres, _ = kmeans.lloyd(torch.from_numpy(big_npy).to(device), kmeans_clusters, kmeans_iterations, seed)
            big_npy = centres.cpu().numpy()

        lists = n_ivf(big_npy.shape[0])
        if lists < 1:
            raise ValueError(f"{big_npy.shape[0]} rows are too few for an IVF index (n_ivf = {lists})")
        index = kmeans.build_ivf_flat_device(big_npy, lists, seed=seed, device=device)
        faiss_index.write_index(index, index_filepath)
        print(f"Saved index file '{index_filepath}'")
        return index_filepath
    except Exception as error:
        print(f"An error occurred extracting the index: {error}")
        print("If you are running this code in a virtual environment, make sure you have enough GPU available to generate the Index file.")
        return None


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if len(argv) != 2:
        print("usage: python -m rvc_amd.train.process.extract_index EXP_DIR {Auto,Faiss,KMeans}")
        return 2
    exp_dir, index_algorithm = str(argv[0]), str(argv[1])
    extract_index(exp_dir, index_algorithm)
    return 1 if not os.path.exists(os.path.join(exp_dir, "extracted")) else 0   # the reference exits 1 only for the missing directory


if __name__ == "__main__":
    sys.exit(main())
