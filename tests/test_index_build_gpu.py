"""The feature-index builder on the MI355X: K16 (rvc_kmeans_assign / rvc_kmeans_update) against float64 NumPy, one Lloyd step
teacher-forced against a float64 restatement of rvc_amd.lib.kmeans' rules, the free-running loop, its clustering quality against
the reference's own reducer (scikit-learn's MiniBatchKMeans, recorded in tests/golden/index_kmeans_sklearn.npz), and
rvc_amd.train.process.extract_index end to end into Pipeline._get_index.

Near-tie rule (the project's own, test_knn_ids_and_distances): a row whose chosen centroid differs from the float64 arg-min is
accepted only when the float64 distance to the chosen centroid exceeds the float64 minimum by at most
8 * 2^-23 * (||x||^2 + ||c||^2), and at most 0.1 % of the rows may be such certified near-ties."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def clustered(seed, n, d, n_centres, jitter):
    r = np.random.default_rng(seed)
    c = r.standard_normal((n_centres, d)).astype(np.float32) * 0.3
    return (c[r.integers(0, n_centres, n)] + r.standard_normal((n, d)).astype(np.float32) * jitter).astype(np.float32)


@pytest.fixture(scope="module")
def N():
    from rvc_amd import _native
    return _native


@pytest.fixture(scope="module")
def KM():
    from rvc_amd.lib import kmeans
    return kmeans


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def d2_matrix64(x, c):
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    return (x64 ** 2).sum(1)[:, None] - 2.0 * x64 @ c64.T + (c64 ** 2).sum(1)[None, :]


def check_assignment(x, c, ids, label=""):
    """ids under the near-tie rule; returns the number of certified near-ties."""
    n = x.shape[0]
    ids = np.asarray(ids).astype(np.int64)
    assert ids.shape == (n,) and (ids >= 0).all() and (ids < c.shape[0]).all(), label
    m = d2_matrix64(x, c)
    ref = m.argmin(1)
    differ = np.nonzero(ids != ref)[0]
    if differ.size:
        xn = (x[differ].astype(np.float64) ** 2).sum(1)
        cn = (c[ids[differ]].astype(np.float64) ** 2).sum(1)
        excess = m[differ, ids[differ]] - m[differ, ref[differ]]
        bound = 8 * 2.0 ** -23 * (xn + cn)
        bad = excess > bound
        assert not bad.any(), f"{label}: {int(bad.sum())} rows chose a centroid that is no near-tie (worst excess {excess.max():.3e}, bound {bound[excess.argmax()]:.3e})"
        assert differ.size <= 0.001 * n, f"{label}: {differ.size} certified near-ties among {n} rows"
    return int(differ.size)


def check_d2(x, c, ids, d2, label=""):
    want = ((x.astype(np.float64) - c[np.asarray(ids).astype(np.int64)].astype(np.float64)) ** 2).sum(1)
    assert d2.dtype == np.float32
    assert np.allclose(d2, want, rtol=1e-5, atol=1e-5), (label, np.abs(d2 - want).max())


def planned_stripes(n, k):
    """csrc/kmeans.hip km_plan: centroid stripes of at least four 128-tiles until (row tiles x stripes) reaches 1024 blocks."""
    row_tiles = -(-n // 128)
    want = max(1, min(-(-1024 // row_tiles), -(-k // 512)))
    stripe = -(-(-(-k // want)) // 128) * 128
    return -(-k // stripe)


def assign_case(n, k, d, seed=11):
    x = clustered(seed, n, d, 40, 0.3)
    r = np.random.default_rng(seed + 1)
    c = (x[r.choice(n, k, replace=k > n)] + 0.01 * r.standard_normal((k, d))).astype(np.float32)
    return x, c


# ---- assign ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,d", [(1, 1, 256), (257, 3, 256), (129, 129, 32), (5000, 130, 768), (70_001, 300, 256), (300, 1100, 64)])
def test_assign_vs_float64(N, n, k, d):
    if (n, k, d) == (300, 1100, 64):
        assert planned_stripes(n, k) == 3            # this is the case with more than one centroid stripe (the last one partial)
    else:
        assert planned_stripes(n, k) == 1
    x, c = assign_case(n, k, d)
    ids, d2 = N.kmeans_assign(dev(x), dev(c))
    assert ids.dtype == torch.int32 and d2.dtype == torch.float32 and ids.shape == (n,) and d2.shape == (n,)
    ids, d2 = ids.cpu().numpy(), d2.cpu().numpy()
    ties = check_assignment(x, c, ids, f"assign {n} x {k} x {d}")
    check_d2(x, c, ids, d2, f"assign {n} x {k} x {d}")
    print(f"assign {n} x {k} x {d}: {ties} certified near-ties, max d2 {d2.max():.4f}")


def test_assign_does_not_depend_on_the_launch_plan(N):
    """The same 300 rows alone (three centroid stripes) and as the head of a matrix long enough for one stripe: same bits."""
    x, c = assign_case(300, 1100, 64)
    n_big = 128 * 1024 + 300
    assert planned_stripes(300, 1100) == 3 and planned_stripes(n_big, 1100) == 1
    big = np.concatenate([x, np.tile(x, (n_big // 300, 1))[:n_big - 300]], 0)
    ids_a, d2_a = N.kmeans_assign(dev(x), dev(c))
    ids_b, d2_b = N.kmeans_assign(dev(big), dev(c))
    assert torch.equal(ids_a, ids_b[:300]) and torch.equal(d2_a.view(torch.int32), d2_b[:300].view(torch.int32))
    # every copy of a row, wherever it sits in its 128-row tile, gets that row's answer
    pos = torch.arange(300, n_big, device=DEV) - 300
    assert torch.equal(ids_b[300:], ids_a[pos % 300]) and torch.equal(d2_b[300:], d2_a[pos % 300])


def test_assign_ties_exact_hits_and_repeatability(N):
    x, c = assign_case(5000, 130, 768)
    c[9] = c[5]                                                   # identical centroids: equal scores go to the lower id
    c[77] = x[1234]                                               # a centroid equal to a row
    m = d2_matrix64(x, c)
    near5 = np.nonzero(m.argmin(1) == 5)[0]
    assert near5.size > 0                                         # centroid 5 (= 9) is the nearest of some rows
    xd, cd = dev(x), dev(c)
    ids, d2 = N.kmeans_assign(xd, cd)
    ids2, d22 = N.kmeans_assign(xd, cd)
    assert torch.equal(ids, ids2) and torch.equal(d2.view(torch.int32), d22.view(torch.int32))
    ids, d2 = ids.cpu().numpy(), d2.cpu().numpy()
    check_assignment(x, c, ids, "ties")
    assert (ids[near5] == 5).all() and not (ids == 9).any()
    assert ids[1234] == 77 and d2[1234] == 0.0
    # the workspace is shared with other shapes in between: still the same bits
    N.kmeans_assign(dev(x[:700]), dev(c[:3]))
    ids3, d23 = N.kmeans_assign(xd, cd)
    assert torch.equal(ids3, ids2) and torch.equal(d23, d22)


# ---- update ---------------------------------------------------------------------------------------------------------------
def members(ids, k):
    order = np.argsort(ids, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=k))]).astype(np.int64)
    return order, offsets


def mean64(x, order, offsets, old):
    """float64 mean over the valid members, `old` where there are none."""
    out = old.astype(np.float64).copy()
    for j in range(old.shape[0]):
        m = order[offsets[j]:offsets[j + 1]]
        m = m[(m >= 0) & (m < x.shape[0])]
        if m.size:
            out[j] = x[m].astype(np.float64).sum(0) / m.size
    return out


def check_update(got, want64, label=""):
    """within one fp32 ulp of the float64 mean, element by element"""
    assert got.dtype == np.float32
    ulp = np.spacing(np.abs(want64.astype(np.float32)))
    err = np.abs(got.astype(np.float64) - want64)
    assert (err <= ulp).all(), (label, float((err / ulp).max()))


def run_update(N, x, order, offsets, old):
    xd, od, fd, cd = dev(x), dev(order), dev(offsets), dev(old)
    a = N.kmeans_update(xd, od, fd, cd)
    b = N.kmeans_update(xd, od, fd, cd)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two calls differ"
    return a.cpu().numpy()


def test_update_random_assignment(N):
    n, k, d = 5000, 130, 768
    x, old = assign_case(n, k, d)
    r = np.random.default_rng(3)
    ids = r.integers(0, k, n)
    ids[ids == 17] = 18                                           # an empty centroid among populated ones
    ids[ids == k - 1] = 0                                         # ... and the last one
    order, offsets = members(ids, k)
    got = run_update(N, x, order, offsets, old)
    check_update(got, mean64(x, order, offsets, old), "random")
    assert np.array_equal(got[17].view(np.int32), old[17].view(np.int32)) and np.array_equal(got[k - 1].view(np.int32), old[k - 1].view(np.int32))


def test_update_one_centroid_owns_every_row(N):
    """the split-list path: 100 000 members are 391 pieces of 256, the last one partial"""
    n, d = 100_000, 256
    x = clustered(5, n, d, 40, 0.3) + np.float32(0.25)           # a non-zero mean, so that the sum grows
    old = np.random.default_rng(6).standard_normal((3, d)).astype(np.float32)
    order = np.random.default_rng(7).permutation(n).astype(np.int32)
    offsets = np.array([0, 0, n, n], dtype=np.int64)
    got = run_update(N, x, order, offsets, old)
    check_update(got, mean64(x, order, offsets, old), "one list")
    assert np.array_equal(got[[0, 2]].view(np.int32), old[[0, 2]].view(np.int32))


def test_update_skips_out_of_range_entries(N):
    n, k, d = 3000, 7, 256
    x, old = assign_case(n, k, d)
    r = np.random.default_rng(8)
    ids = r.integers(0, k - 1, n)
    ids[:700] = 2                                                 # a list of more than two pieces
    order, offsets = members(ids, k)
    bad = r.choice(n, 400, replace=False)
    order[bad] = r.choice(np.array([-1, -7, n, n + 5, 2 ** 31 - 1, -2 ** 31], dtype=np.int64), 400).astype(np.int32)
    lo, hi = offsets[4], offsets[5]
    order[lo:hi] = -1                                             # a list whose every entry is skipped keeps the old centroid
    got = run_update(N, x, order, offsets, old)
    check_update(got, mean64(x, order, offsets, old), "skips")
    assert np.array_equal(got[4].view(np.int32), old[4].view(np.int32)) and np.array_equal(got[6].view(np.int32), old[6].view(np.int32))


# ---- one Lloyd step, teacher-forced ---------------------------------------------------------------------------------------
def restated_step(x, c):
    """rvc_amd.lib.kmeans.lloyd_step in float64 NumPy on float32 centroids: -> (new centroids float32, ids, d2, re-seeded)."""
    k = c.shape[0]
    ids = d2_matrix64(x, c).argmin(1)
    d2 = ((x.astype(np.float64) - c[ids].astype(np.float64)) ** 2).sum(1)
    order, offsets = members(ids, k)
    new = mean64(x, order, offsets, c).astype(np.float32)
    empty = np.nonzero(np.diff(offsets) == 0)[0]                  # ascending id
    far = np.argsort(-d2, kind="stable")[:empty.size]             # largest d2 first, ties: the lower row
    new[empty] = x[far]
    return new, ids, d2, empty.size


@pytest.mark.parametrize("jitter,expect_reseed", [(0.3, False), (0.05, True)])
def test_lloyd_step_teacher_forced(KM, jitter, expect_reseed):
    x = clustered(7, 6000, 256, 400, jitter)
    k = 153
    xd = dev(x)
    c = x[np.random.default_rng(0).choice(6000, k, replace=False)].copy()
    reseeds = 0
    for it in range(10):
        want, ids_r, d2_r, n_empty = restated_step(x, c)
        reseeds += n_empty
        got, ids, d2 = KM.lloyd_step(xd, dev(c))
        ties = check_assignment(x, c, ids.cpu().numpy(), f"iteration {it}")
        got = got.cpu().numpy()
        print(f"jitter {jitter} iteration {it}: {ties} near-ties, {n_empty} empty, max centroid error "
              f"{np.abs(got - want).max():.3e}, inertia {d2_r.sum():.6f}")
        assert np.allclose(got, want, rtol=1e-5, atol=1e-8), (it, np.abs(got - want).max())
        assert abs(float(d2.double().sum()) - d2_r.sum()) <= 1e-5 * d2_r.sum()
        c = want
    if expect_reseed:
        assert reseeds >= 1, "this data set is here to exercise the re-seed rule"
    else:
        assert reseeds == 0, "precondition: no empty cluster on this data"


# ---- free-running ---------------------------------------------------------------------------------------------------------
def test_lloyd_is_reproducible_and_inertia_never_rises(KM):
    for jitter in (0.3, 0.05):
        xd = dev(clustered(7, 6000, 256, 400, jitter))
        c1, i1 = KM.lloyd(xd, 153, 10, 0)
        c2, i2 = KM.lloyd(xd, 153, 10, 0)
        assert c1.shape == (153, 256) and c1.dtype == torch.float32 and len(i1) == 10
        assert torch.equal(c1.view(torch.int32), c2.view(torch.int32)) and i1 == i2
        print(f"jitter {jitter}: inertia", " ".join(f"{v:.4f}" for v in i1))
        for a, b in zip(i1, i1[1:]):
            assert b <= a * (1 + 1e-6), i1
        c3, _ = KM.lloyd(xd, 153, 10, 1)
        assert not torch.equal(c1, c3)                            # another seed, another start


def test_quality_against_the_reference_reducer(KM):
    g = np.load(os.path.join(GOLDEN, "index_kmeans_sklearn.npz"), allow_pickle=False)
    seed, n, d, n_centres, jitter = g["recipe"]
    x = clustered(int(seed), int(n), int(d), int(n_centres), float(jitter))
    assert x.astype(np.float64).sum() == float(g["data_sum"]), "the recipe no longer regenerates the fixture's data"
    ref = g["inertias"]
    median = float(np.median(ref))
    m = 2.0 * float(ref.max() - ref.min()) / median
    c, per_iteration = KM.lloyd(dev(x), int(g["k"]), 20, 0)
    inertia = float(d2_matrix64(x, c.cpu().numpy()).min(1).sum())
    print(f"lloyd inertia {inertia:.3f} (start {per_iteration[0]:.3f}); sklearn median {median:.3f}, m = {m:.5f}, gate {(1 + m) * median:.3f}")
    assert inertia <= (1 + m) * median


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _write_exp(tmp_path, name, x):
    exp = tmp_path / name
    (exp / "extracted").mkdir(parents=True)
    for i, part in enumerate(np.array_split(x, 3)):
        np.save(exp / "extracted" / f"{i}_feats.npy", part)
    return str(exp)


def _sorted_rows(a):
    rows = np.ascontiguousarray(a).view(np.dtype((np.void, a.shape[1] * 4))).ravel()
    return np.sort(rows)


def test_extract_index_end_to_end(KM, tmp_path):
    from rvc_amd.configs.config import Config
    from rvc_amd.infer.pipeline import FeatureIndex, Pipeline
    from rvc_amd.lib import faiss_index as FI
    from rvc_amd.train.process.extract_index import extract_index
    x = clustered(7, 6000, 768, 400, 0.3)
    exp = _write_exp(tmp_path, "voice", x)
    path = extract_index(exp, "Auto", device=DEV, seed=3)
    assert path == os.path.join(exp, "voice.index") and os.path.isfile(path)
    ivf = FI.read_index(path)
    assert (ivf.nlist, ivf.nprobe, ivf.ntotal, ivf.d) == (153, 1, 6000, 768)
    big = ivf.reconstruct_n(0, 6000)
    assert np.array_equal(_sorted_rows(big), _sorted_rows(x))                        # a permutation of the input rows
    assert np.array_equal(big, x[np.random.default_rng(3).permutation(6000)])        # ... the seeded shuffle
    list_of = np.full(6000, -1, dtype=np.int64)
    for j, ids in enumerate(ivf.list_ids):
        assert (np.diff(ids) > 0).all()                                              # ascending inside a list
        list_of[ids] = j
    check_assignment(big, ivf.centroids, list_of, "inverted lists")                  # every row in its nearest centroid's list
    for ids, vecs in zip(ivf.list_ids, ivf.list_vecs):
        assert np.array_equal(vecs, big[ids])

    # a second call does nothing
    stamp = os.stat(path)
    assert extract_index(exp, "Auto", device=DEV, seed=4) == path
    after = os.stat(path)
    assert (after.st_mtime_ns, after.st_size) == (stamp.st_mtime_ns, stamp.st_size)

    # the file through the pipeline's loader
    pipe = Pipeline(48000, Config(DEV))
    r = np.random.default_rng(1)
    q = (big[r.integers(0, 6000, 200)] + 0.03 * r.standard_normal((200, 768))).astype(np.float32)
    index = pipe._get_index(path, 0.75)
    assert index is not None and index.search_mode == "exact" and index.ntotal == 6000
    d_ex, i_ex = index.search(q, 8)
    d_fi, i_fi = FeatureIndex(big, DEV).search(q, 8)
    assert np.array_equal(i_ex, i_fi) and np.array_equal(d_ex, d_fi)
    pipe.index_search = "ivf"
    pipe._index_cache = {}
    index = pipe._get_index(path, 0.75)
    assert index.search_mode == "ivf"
    _, i_ivf = index.search(q, 8)
    probed = np.where(i_ivf >= 0, list_of[np.clip(i_ivf, 0, None)], -1)
    assert (i_ivf[:, 0] >= 0).all()
    assert ((probed == probed[:, :1]) | (i_ivf < 0)).all()                           # only members of ONE list per query ...
    check_assignment(q, ivf.centroids, probed[:, 0], "probed list")                  # ... the nearest centroid's


def test_extract_index_reduction_and_faiss(tmp_path):
    from rvc_amd.lib import faiss_index as FI
    from rvc_amd.train.process.extract_index import extract_index
    x = clustered(7, 6000, 256, 400, 0.3)
    kw = dict(device=DEV, seed=3, kmeans_threshold=4000, kmeans_clusters=300)
    ivf = FI.read_index(extract_index(_write_exp(tmp_path, "reduced", x), "Auto", **kw))
    assert (ivf.ntotal, ivf.nlist, ivf.nprobe, ivf.d) == (300, 7, 1, 256)
    centres = ivf.reconstruct_n(0, 300)
    assert np.isfinite(centres).all() and np.unique(centres, axis=0).shape[0] == 300
    # the centres are k-means centres of the data: far less inertia than 300 rows picked at random
    picked = x[np.random.default_rng(0).choice(6000, 300, replace=False)]
    assert d2_matrix64(x, centres).min(1).sum() < 0.9 * d2_matrix64(x, picked).min(1).sum()
    ivf = FI.read_index(extract_index(_write_exp(tmp_path, "plain", x), "Faiss", **kw))
    assert (ivf.ntotal, ivf.nlist, ivf.nprobe) == (6000, 153, 1)
    assert np.array_equal(_sorted_rows(ivf.reconstruct_n(0, 6000)), _sorted_rows(x))
