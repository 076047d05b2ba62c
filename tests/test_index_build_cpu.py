"""The feature-index builder without a device: the K16 entries of the C ABI (rvc_kmeans_workspace_bytes / _assign / _update) refuse
every bad argument of their contract before anything touches a device, and the host logic of
rvc_amd.train.process.extract_index follows the reference's extract_index.py (n_ivf, skip-if-exists, the missing-directory
message and status, "Faiss" never reduces, the two positional CLI arguments).  The clustering itself runs in
test_index_build_gpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, PKG, REPO

P = 0x10000          # a plausible, 16-byte aligned, never dereferenced "device pointer"
BIG = 1 << 31


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()                                    # the library may not exist yet when this file runs alone
    from rvc_amd import _native
    return _native._lib


def _plant_other_error(lib):
    need = ctypes.c_size_t()
    assert lib.rvc_knn_workspace_bytes(100, 10, 768, 5, ctypes.byref(need)) != 0
    assert b"k must be 8" in lib.rvc_last_error()


def _refused(lib, name, *args):
    _plant_other_error(lib)
    rc = getattr(lib, name)(*args)
    msg = lib.rvc_last_error()
    assert rc != 0, (name, args, "accepted")
    assert msg.startswith(name.encode() + b": ") and len(msg) > len(name) + 2, (name, args, msg)
    return msg


BAD_SHAPES = [  # (n_rows, n_centroids, dim)
    (100, 10, 0), (100, 10, 16), (100, 10, 31), (100, 10, 33), (100, 10, 48), (100, 10, 767), (100, 10, 1056), (100, 10, 2048),
    (100, 10, -32), (100, 0, 768), (100, -1, 768), (-1, 10, 768), (BIG, 10, 768), (100, BIG, 768), (1 << 40, 10, 768),
]


def test_workspace_bytes_contract(lib):
    need = ctypes.c_size_t()
    for n, k, d in BAD_SHAPES:
        _refused(lib, "rvc_kmeans_workspace_bytes", n, k, d, ctypes.byref(need))
    _refused(lib, "rvc_kmeans_workspace_bytes", 100, 10, 768, None)
    for n, k, d in [(0, 1, 32), (1, 1, 256), (100, 10, 768), (BIG - 1, BIG - 1, 1024), (2_000_000, 10_000, 768)]:
        need.value = 0
        assert lib.rvc_kmeans_workspace_bytes(n, k, d, ctypes.byref(need)) == 0, (n, k, d, lib.rvc_last_error())
        assert need.value > 0
    # two million rows are one call, in O(n_rows) words: not rvc_knn_search's 42 KB per query
    assert lib.rvc_kmeans_workspace_bytes(2_000_000, 10_000, 768, ctypes.byref(need)) == 0
    assert need.value < 2_000_000 * 64, need.value


def test_assign_refuses_bad_arguments_before_any_device_call(lib):
    need = ctypes.c_size_t()
    assert lib.rvc_kmeans_workspace_bytes(100, 10, 768, ctypes.byref(need)) == 0
    ws = need.value

    def call(x=P, n=100, d=768, c=P, k=10, ids=P, d2=P, w=P, wb=ws):
        return ("rvc_kmeans_assign", x, n, d, c, k, ids, d2, w, wb, None)

    for kw in ({"x": None}, {"c": None}, {"ids": None}, {"d2": None}, {"w": None}):
        assert b"null pointer" in _refused(lib, *call(**kw))
    for n, k, d in BAD_SHAPES:
        _refused(lib, *call(n=n, k=k, d=d, wb=1 << 62))
    assert b"workspace too small" in _refused(lib, *call(wb=ws - 1))
    assert b"workspace too small" in _refused(lib, *call(wb=0))
    assert b"workspace too small" in _refused(lib, *call(n=0, wb=0))      # checked even when there is nothing to launch
    # n_rows == 0 with good arguments: status 0, nothing launched (there is no device here to launch on)
    assert lib.rvc_kmeans_assign(P, 0, 768, P, 10, P, P, P, ws, None) == 0, lib.rvc_last_error()


def test_update_refuses_bad_arguments_before_any_device_call(lib):
    need = ctypes.c_size_t()
    assert lib.rvc_kmeans_workspace_bytes(100, 10, 768, ctypes.byref(need)) == 0
    ws = need.value

    def call(x=P, n=100, d=768, order=P, off=P, k=10, old=P, out=P, w=P, wb=ws):
        return ("rvc_kmeans_update", x, n, d, order, off, k, old, out, w, wb, None)

    for kw in ({"x": None}, {"order": None}, {"off": None}, {"old": None}, {"out": None}, {"w": None}):
        assert b"null pointer" in _refused(lib, *call(**kw))
    for n, k, d in BAD_SHAPES:
        _refused(lib, *call(n=n, k=k, d=d, wb=1 << 62))
    assert b"workspace too small" in _refused(lib, *call(wb=ws // 2))
    assert b"workspace too small" in _refused(lib, *call(wb=0))
    assert lib.rvc_kmeans_update(P, 0, 768, P, P, 10, P, P, P, ws, None) == 0, lib.rvc_last_error()


# ---- the tool -------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def tool(lib):
    from rvc_amd.train.process import extract_index as T
    return T


def test_n_ivf_formula(tool):
    assert [tool.n_ivf(n) for n in (39, 40, 6000, 100_000, 200_001, 2_000_000)] == [1, 1, 153, 2564, 5128, 22627]


def _exp_dir(tmp_path, rows=120, d=256, name="voice"):
    exp = tmp_path / name
    (exp / "extracted").mkdir(parents=True)
    r = np.random.default_rng(5)
    x = r.standard_normal((rows, d)).astype(np.float32)
    for i, part in enumerate(np.array_split(x, 3)):
        np.save(exp / "extracted" / f"{2 - i}_part.npy", part)       # sorted(listdir) order is the reverse of write order
    return exp, np.concatenate([p for p in reversed(np.array_split(x, 3))], 0)


def test_missing_directory_message_and_status(tool, tmp_path, capsys):
    exp = tmp_path / "nothing_here"
    exp.mkdir()
    assert tool.extract_index(str(exp), "Auto") is None
    want = (f"Feature to generate index file not found at {os.path.join(str(exp), 'extracted')}. "
            "Did you run preprocessing and feature extraction steps?")
    assert capsys.readouterr().out.strip() == want
    assert tool.main([str(exp), "Auto"]) == 1
    assert capsys.readouterr().out.strip() == want
    assert not os.path.exists(exp / "nothing_here.index")


def test_skip_if_index_exists(tool, tmp_path, monkeypatch, capsys):
    exp, _ = _exp_dir(tmp_path)
    target = exp / "voice.index"
    target.write_bytes(b"already here")

    def boom(*a, **k):
        raise AssertionError("nothing may be built when the index file exists")

    monkeypatch.setattr(tool.kmeans, "build_ivf_flat_device", boom)
    monkeypatch.setattr(tool.kmeans, "lloyd", boom)
    assert tool.extract_index(str(exp), "Auto") == str(target)
    assert target.read_bytes() == b"already here" and capsys.readouterr().out == ""
    assert tool.main([str(exp), "Auto"]) == 0


def _fake_builder(calls):
    from rvc_amd.lib import faiss_index as FI

    def build(big_npy, nlist, seed=0, iterations=10, device="cuda:0"):
        calls.append((np.array(big_npy, copy=True), nlist, seed, device))
        return FI.build_ivf_flat(big_npy, nlist, seed=0, iterations=1)
    return build


def test_faiss_never_reduces_and_auto_does(tool, tmp_path, monkeypatch, capsys):
    import torch
    from rvc_amd.lib import faiss_index as FI
    exp, x = _exp_dir(tmp_path)
    built, reduced = [], []

    def fake_lloyd(x_dev, k, iterations, seed):
        reduced.append((tuple(x_dev.shape), k, iterations, seed))
        return x_dev[:k].clone(), [0.0] * iterations

    monkeypatch.setattr(tool.kmeans, "build_ivf_flat_device", _fake_builder(built))
    monkeypatch.setattr(tool.kmeans, "lloyd", fake_lloyd)
    kw = dict(device="cpu", seed=3, kmeans_threshold=100, kmeans_clusters=80, kmeans_iterations=4)
    path = tool.extract_index(str(exp), "Faiss", **kw)
    assert path == str(exp / "voice.index") and reduced == []
    big, nlist, seed, device = built.pop()
    assert big.shape == (120, 256) and nlist == 3 and seed == 3 and device == "cpu"
    assert np.array_equal(big, x[np.random.default_rng(3).permutation(120)])        # sorted file order, then the seeded shuffle
    assert capsys.readouterr().out.strip() == f"Saved index file '{path}'"
    ivf = FI.read_index(path)
    assert (ivf.ntotal, ivf.nlist, ivf.nprobe) == (120, 3, 1)
    for algorithm in ("Auto", "KMeans"):
        os.remove(path)
        assert tool.extract_index(str(exp), algorithm, **kw) == path
        assert reduced.pop() == ((120, 256), 80, 4, 3)
        big, nlist, _, _ = built.pop()
        assert big.shape == (80, 256) and nlist == 2
    # at or below the threshold nothing is reduced either
    os.remove(path)
    assert tool.extract_index(str(exp), "Auto", **{**kw, "kmeans_threshold": 120}) == path and reduced == []
    assert built.pop()[0].shape == (120, 256)


def test_errors_are_printed_in_the_reference_words_and_swallowed(tool, tmp_path, capsys):
    exp = tmp_path / "odd"
    (exp / "extracted").mkdir(parents=True)
    np.save(exp / "extracted" / "a.npy", np.zeros((50, 100), np.float32))           # 100 is no index dimension
    assert tool.extract_index(str(exp), "Auto", device="cpu") is None
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("An error occurred extracting the index: ") and "256, 512, 768, 1024" in out[0]
    assert out[1] == ("If you are running this code in a virtual environment, make sure you have enough GPU available to "
                      "generate the Index file.")
    assert tool.main([str(exp), "Auto"]) == 0                                        # the reference exits 0 here


def test_cli_argument_order(tool, tmp_path, monkeypatch):
    seen = []
    monkeypatch.setattr(tool, "extract_index", lambda exp_dir, algorithm="Auto", **kw: seen.append((exp_dir, algorithm, kw)))
    (tmp_path / "extracted").mkdir()
    assert tool.main([str(tmp_path), "KMeans"]) == 0
    assert seen == [(str(tmp_path), "KMeans", {})]
    assert tool.main([str(tmp_path)]) == 2 and tool.main([]) == 2 and len(seen) == 1
    # the module as a program: EXP_DIR first, the algorithm second; a missing extracted/ is exit status 1
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO, os.environ.get("PYTHONPATH", "")]))
    exp = tmp_path / "cli"
    exp.mkdir()
    run = subprocess.run([sys.executable, "-m", "rvc_amd.train.process.extract_index", str(exp), "Auto"], env=env,
                         capture_output=True, text=True)
    assert run.returncode == 1, run.stderr
    assert run.stdout.strip().startswith(f"Feature to generate index file not found at {os.path.join(str(exp), 'extracted')}.")


def test_sklearn_fixture_shape():
    g = np.load(os.path.join(GOLDEN, "index_kmeans_sklearn.npz"), allow_pickle=False)
    assert tuple(g["recipe"]) == (0, 20480, 256, 512, 0.05) and int(g["k"]) == 128
    assert g["inertias"].shape == (5,) and g["inertias"].dtype == np.float64 and list(g["seeds"]) == [0, 1, 2, 3, 4]
    assert np.isfinite(g["inertias"]).all() and (g["inertias"] > 0).all()
    assert g["data_sum"].dtype == np.float64 and g["data_sum"].shape == ()
