"""Lloyd's k-means on the device (K16: rvc_kmeans_assign / rvc_kmeans_update) and the IVF index built from it.

The reference clusters on the CPU: ``MiniBatchKMeans(n_clusters=10000)`` when ``big_npy`` has more than 2e5 rows, then faiss'
own k-means inside ``index.train`` for the ``IVF{n_ivf},Flat`` coarse quantiser and ``index.add`` for the inverted lists
(rvc/train/process/extract_index.py:43-69).  Here both are plain Lloyd iterations whose two heavy steps are native kernels; the
host (torch) only sorts the assignment, turns it into list offsets and re-seeds empty clusters.  Bit-parity with faiss' or
scikit-learn's centroids is not a goal: both are unseeded in the reference, and any centroid set gives a valid index.
"""
from __future__ import annotations

import numpy as np
import torch

from rvc_amd import _native
from rvc_amd.lib.faiss_index import IVFFlatIndex


def _sorted_members(ids: torch.Tensor, k: int):
    """ids int32 [n] -> (order int32 [n]: rows sorted by centroid, row order kept inside one; offsets int64 [k + 1]; counts)."""
    ids64 = ids.to(torch.int64)
    order = torch.argsort(ids64, stable=True).to(torch.int32)
    counts = torch.bincount(ids64, minlength=k)
    offsets = torch.zeros(k + 1, dtype=torch.int64, device=ids.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return order, offsets, counts


def lloyd_step(x: torch.Tensor, centroids: torch.Tensor):
    """One iteration from ``centroids``: assign, sort, offsets, update, re-seed.  -> (new centroids, ids, d2).

    Empty clusters are re-seeded deterministically: the e-th empty centroid, in ascending id, takes the row with the e-th
    largest d2 of this assignment (ties: the lower row id)."""
    k = centroids.shape[0]
    ids, d2 = _native.kmeans_assign(x, centroids)
    order, offsets, counts = _sorted_members(ids, k)
    new = _native.kmeans_update(x, order, offsets, centroids)
    empty = torch.nonzero(counts == 0).flatten()
    if empty.numel():
        far = torch.sort(d2, descending=True, stable=True).indices[:empty.numel()]
        new[empty] = x[far]
    return new, ids, d2


def lloyd(x_dev: torch.Tensor, k: int, iterations: int, seed):
    """``iterations`` Lloyd iterations (a fixed count, no early stop) over the rows of ``x_dev`` [n, d] (float32, in HBM).

    Init: ``x[np.random.default_rng(seed).choice(n, k, replace=False)]``, the rule ``faiss_index.build_ivf_flat`` uses.
    -> (centroids [k, d] float32 on the device, inertia_per_iteration): ``inertia_per_iteration[i]`` is the float64 sum of the
    squared distances of iteration i's assignment, i.e. the inertia of the centroids that iteration started from."""
    if x_dev.dim() != 2 or not x_dev.is_cuda or x_dev.dtype != torch.float32:
        raise _native.NativeError("lloyd: x_dev must be a float32 [n, d] tensor in HBM (there is no CPU path)")
    n = x_dev.shape[0]
    k = int(k)
    if not 1 <= k <= n:
        raise ValueError(f"lloyd: k = {k} centroids from {n} rows")
    x_dev = x_dev.contiguous()
    pick = np.random.default_rng(seed).choice(n, k, replace=False)
    centroids = x_dev[torch.from_numpy(np.asarray(pick, dtype=np.int64)).to(x_dev.device)].contiguous()
    inertia = []
    for _ in range(int(iterations)):
        centroids, _, d2 = lloyd_step(x_dev, centroids)
        inertia.append(d2.to(torch.float64).sum())
    return centroids, [float(v) for v in inertia]


def build_ivf_flat_device(big_npy: np.ndarray, nlist: int, seed=0, iterations: int = 10, device="cuda:0") -> IVFFlatIndex:
    """``index.train`` + ``index.add`` of an ``IVF{nlist},Flat`` index (extract_index.py:62-69) on the device: ``lloyd`` for the
    coarse centroids, one last assignment, then every row into the list of its nearest centroid under its row position in
    ``big_npy`` (add order), ids ascending inside a list, ``nprobe = 1`` -- the object ``faiss_index.build_ivf_flat`` returns.

    ``iterations = 10`` is faiss' ``niter`` for an IVF coarse quantiser.  faiss would also subsample the training set above 256
    points per centroid; with the reference's ``n_ivf = min(16 sqrt(N), N // 39)`` that only happens above 16.7 M rows, so
    there is no subsampling here."""
    x = np.ascontiguousarray(big_npy, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError(f"big_npy must be [N, d], got {x.shape}")
    n, d = x.shape
    nlist = int(max(1, min(nlist, n)))
    x_dev = torch.from_numpy(x).to(device)
    centroids, _ = lloyd(x_dev, nlist, iterations, seed)
    ids, _ = _native.kmeans_assign(x_dev, centroids)
    a = ids.cpu().numpy().astype(np.int64)
    order = np.argsort(a, kind="stable")
    bounds = np.searchsorted(a[order], np.arange(nlist + 1))
    lists = [order[bounds[j]:bounds[j + 1]].astype(np.int64) for j in range(nlist)]
    return IVFFlatIndex(d, centroids.cpu().numpy(), lists, [x[i] for i in lists], nprobe=1)
