"""LPIPS on the host side: the float64 restatement pinned, the weight loader, and the sweep's argument checks / CSV layout."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_reference as R  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402
S = importlib.import_module("adaptive_edge_aware_jpeg_amd.sweep")


@pytest.fixture(scope="module")
def sd():
    return R.random_state_dicts(7)


def _pair(h, w, seed, noise=0.05):
    g = np.random.default_rng(seed)
    x = g.random((h, w, 3)).astype(np.float32)
    y = np.clip(x + noise * g.standard_normal(x.shape), 0, 1).astype(np.float32)
    return x, y


def test_reference_identity_symmetry_and_size_boundary(sd):
    alex, lin = sd
    x, y = _pair(31, 31, 1)
    assert R.lpips64(x, x, alex, lin) == 0.0
    d = R.lpips64(x, y, alex, lin)
    assert d > 0 and R.lpips64(y, x, alex, lin) == pytest.approx(d, rel=1e-12)
    with pytest.raises(ValueError):
        R.lpips64(x[:30], y[:30], alex, lin)
    import torch
    import torch.nn.functional as F
    with pytest.raises(RuntimeError):        # what the reference's torch does at 30: the second maxpool has no output
        t = F.relu(F.conv2d(torch.zeros(1, 3, 30, 30), alex["features.0.weight"], stride=4, padding=2))
        F.max_pool2d(F.relu(F.conv2d(F.max_pool2d(t, 3, 2), alex["features.3.weight"], padding=2)), 3, 2)


@pytest.mark.parametrize("h,w", [(31, 37), (40, 33)])
def test_reference_matches_loop_restatement(sd, h, w):
    alex, lin = sd
    x, y = _pair(h, w, h * w)
    assert R.lpips64(x, y, alex, lin) == pytest.approx(R.lpips_loops(x, y, alex, lin), rel=1e-10, abs=1e-13)


def test_loader_layouts_pack_identically(sd, tmp_path):
    import torch
    alex, lin = sd
    a = A.LpipsWeights.load(alex, lin)
    b = A.LpipsWeights.load(R.lpips_state_dict(alex, lin))
    torch.save(alex, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "alex.pth")
    c = A.LpipsWeights.load(str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth"))
    pa = a.packed_host()
    assert pa.size == A._lib.load_library().aej_lpips_weights_bytes() and np.any(pa)
    assert np.array_equal(pa, b.packed_host()) and np.array_equal(pa, c.packed_host())
    assert a.params().size == A._lib.load_library().aej_lpips_param_count()


def test_packed_layout(sd):
    """[K][Cout] per layer, K = (ky * k + kx) * CinP + c, conv1's channels padded to 4 with zeros"""
    alex, lin = sd
    p = A.LpipsWeights.load(alex, lin).packed_host().view(np.float32)
    w1 = alex["features.0.weight"].numpy()
    k1 = p[:11 * 11 * 4 * 64].reshape(11, 11, 4, 64)
    assert np.array_equal(k1[:, :, :3, :], w1.transpose(2, 3, 1, 0)) and not np.any(k1[:, :, 3, :])
    assert np.array_equal(p[11 * 11 * 4 * 64:11 * 11 * 4 * 64 + 64], alex["features.0.bias"].numpy())


def test_loader_errors_name_the_key(sd):
    import torch
    alex, lin = sd
    bad = dict(alex)
    del bad["features.6.bias"]
    with pytest.raises(ValueError, match="features.6.bias"):
        A.LpipsWeights.load(bad, lin)
    bad = dict(alex)
    bad["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match="features.3.weight"):
        A.LpipsWeights.load(bad, lin)
    bad = dict(lin)
    w = bad["lin2.model.1.weight"].clone()
    w[0, 5, 0, 0] = float("nan")
    bad["lin2.model.1.weight"] = w
    with pytest.raises(ValueError, match="lin2.model.1.weight"):
        A.LpipsWeights.load(alex, bad)
    with pytest.raises(ValueError, match="lin0.model.1.weight"):
        A.LpipsWeights.load(alex)                          # torchvision dict alone: no lin layers
    full = R.lpips_state_dict(alex, lin)
    del full["net.slice5.10.weight"]
    with pytest.raises(ValueError, match="net.slice5.10.weight"):
        A.LpipsWeights.load(full)
    full = R.lpips_state_dict(alex, lin)
    full["scaling_layer.scale"] = full["scaling_layer.scale"] * 2
    with pytest.raises(ValueError, match="scaling_layer.scale"):
        A.LpipsWeights.load(full)
    assert A.LpipsWeights.load(R.lpips_state_dict(alex, lin, scaling=False)) is not None


def test_lpips_without_weights_still_raises():
    assert A.EvaluationMetrics.lpips_weights is None
    x = np.zeros((40, 40, 3), np.float32)
    with pytest.raises(NotImplementedError):
        A.EvaluationMetrics(A.Image.from_array(x), A.Image.from_array(x)).lpips()


def test_sweep_lpips_too_small_raises_before_device_work(sd, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the size check")
    monkeypatch.setattr(S, "get_context", no_device)
    w = A.LpipsWeights.load(*sd)
    with pytest.raises(ValueError, match="31x31"):
        S.sweep(np.zeros((1, 30, 64, 3), np.float32), metrics=S.PSNR, sizes=None, lpips=w)
    with pytest.raises(TypeError):
        S.sweep(np.zeros((1, 64, 64, 3), np.float32), metrics=S.PSNR, sizes=None, lpips="alex.pth")


def test_sweep_csv_lpips_column(tmp_path):
    cells = [("YCbCr", (10, 50), (4, 64)), ("YCbCr", (50, 90), (4, 64))]
    res = S.SweepResult(cells, ["a.png"], [(200, 300)], S.PSNR, "zlib", lpips=True)
    res.psnr[:] = 30.0
    res.lpips[:] = [[0.123456, 0.5]]
    res.bytes[:] = 1000
    res.compression_ratio[:] = 180.0
    rows = res.rows()
    assert list(rows[0]) == list(S.CSV_COLUMNS_LPIPS)
    assert list(S.CSV_COLUMNS_LPIPS[6:]) == ["psnr", "ssim", "ms_ssim", "lpips", "compression_ratio"]
    p = tmp_path / "l.csv"
    res.to_csv(p)
    lines = p.read_text().splitlines()
    assert lines[0] == "image_name,color_space,min_quality,max_quality,min_block_size,max_block_size,psnr,ssim,ms_ssim,lpips,compression_ratio"
    assert lines[1] == "a.png,YCbCr,10,50,4,64,30.0000,nan,nan,0.1235,180.0000"
    plain = S.SweepResult(cells, ["a.png"], [(200, 300)], S.PSNR, "zlib")
    plain.psnr[:] = 30.0
    plain.bytes[:] = 1000
    plain.compression_ratio[:] = 180.0
    q = tmp_path / "p.csv"
    plain.to_csv(q)
    lines = q.read_text().splitlines()
    assert plain.lpips is None and "lpips" not in plain.rows()[0]
    assert lines[0] == ",".join(S.CSV_COLUMNS) and lines[1] == "a.png,YCbCr,10,50,4,64,30.0000,nan,nan,180.0000"


def test_size_functions():
    lib = A._lib.load_library()
    assert lib.aej_lpips_workspace_bytes(1, 30, 64) == 0 and lib.aej_lpips_features_bytes(1, 64, 30) == 0
    f1 = lib.aej_lpips_features_bytes(1, 2160, 3840)
    # the five taps of a 4K image: 539 x 959 x 64, 269 x 479 x 192, 3 x 134 x 239 x (384, 256, 256) floats (each rounded up to 64)
    n = [539 * 959 * 64, 269 * 479 * 192, 134 * 239 * 384, 134 * 239 * 256, 134 * 239 * 256]
    assert f1 == 4 * sum((v + 63) // 64 * 64 for v in n)
    assert lib.aej_lpips_features_bytes(8, 2160, 3840) == 8 * f1
    assert lib.aej_lpips_workspace_bytes(2, 31, 31) > 0
