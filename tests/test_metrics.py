"""EvaluationMetrics (evaluation_metrics.py:50-89): the numpy restatement of piq / cv2 (CPU tests) and the
HIP kernels against it (GPU tests, stated float tolerance -- torch leaves the reduction order of these scores undefined)."""
import numpy as np
import pytest

from oracle import metrics_oracle as M

SSIM_TOL = 1e-4        # absolute, on scores in [0, 1]: sigma = E[x^2] - mu^2 cancels in float32 (piq's type and ours); the restatement uses float64
PSNR_TOL = 1e-4        # dB: the float32 squared differences are within 16 u relative (tests/test_gpu_metrics.py), 7e-5 dB


def pair(oracle, H, W, seed, sigma=0.03):
    a = oracle.synth_image(H, W, seed, "mixed").astype(np.float32) / np.float32(255.0)
    rng = np.random.default_rng(seed)
    b = np.clip(a + rng.normal(0, sigma, a.shape).astype(np.float32), 0, 1).astype(np.float32)
    return a, b


# ------------------------------------------------------------------ CPU: the restatement itself
def test_oracle_grey_and_window():
    u8 = np.array([[[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [12, 200, 77]]], np.uint8)
    assert M.rgb2gray_u8(u8).tolist() == [[255, 76, 150, 29, 130]]          # 0.299 / 0.587 / 0.114 in 14-bit fixed point
    w = M.gaussian_window()
    assert w.shape == (11, 11) and w.dtype == np.float32 and abs(float(w.sum()) - 1.0) < 1e-6
    assert np.array_equal(w, w.T) and np.array_equal(w, w[::-1, ::-1]) and w[5, 5] == w.max()


def test_oracle_psnr_known_values(oracle):
    a = np.full((32, 40, 3), 0.5, np.float32)
    b = a.copy(); b[..., 0] += np.float32(0.1)
    assert abs(M.psnr(a, b) - (-10 * np.log10(0.01 / 3 + 1e-8))) < 1e-5
    assert abs(M.psnr(a, a) - 80.0) < 1e-9                                    # -10 log10(EPS)


def test_oracle_ssim_properties(oracle):
    a, b = pair(oracle, 180, 200, 5)
    assert M.ssim(a, a) == pytest.approx(1.0, abs=1e-12) and M.ms_ssim(a, a) == pytest.approx(1.0, abs=1e-12)
    s1, s2 = M.ssim(a, b), M.ssim(*pair(oracle, 180, 200, 5, sigma=0.1))
    assert 0 < s2 < s1 < 1
    assert M.ssim(a, b) == pytest.approx(M.ssim(b, a), abs=1e-12)
    with pytest.raises(ValueError):
        M.ms_ssim(a[:160], b[:160])
    with pytest.raises(ValueError):
        M.ssim(a[:10], b[:10])


# Every parity of the MS-SSIM pad chain (scale sizes (h % 2, w % 2) = (0, 0), (0, 1), (1, 0), (1, 1) at the pooling steps) and f = 1, 2, 3
DEF_VS_FAST = [(161, 161), (162, 163), (163, 162), (176, 200), (322, 323), (384, 401), (770, 700)]


@pytest.mark.parametrize("H,W", DEF_VS_FAST, ids=[f"{h}x{w}" for h, w in DEF_VS_FAST])
def test_fast_reference_matches_definition(oracle, H, W):
    """The separable float64 restatement against the 2-D one.  With the 1-D taps scaled so that g g^T has the sum of piq's float32
    2-D window, what is left of the window difference is a zero-sum perturbation of at most rho relative per entry (rho from the windows
    themselves, about 5.7e-7); M.ssim_stats(rho=...) turns that and the definition's float32 rounding of pooled inputs into a bound per
    score (first order, no float32 arithmetic on the fast side)."""
    w32 = M.gaussian_window().astype(np.float64)
    g = M.gaussian_1d() * np.sqrt(w32.sum())
    rho = float(np.abs(w32 / np.outer(g, g) - 1).max())
    assert rho < 1e-6
    a, b = pair(oracle, H, W, H * 7 + W)
    f = M.grey_pool_factor(H, W)
    assert f == {770: 3, 384: 2}.get(H, 1)
    s, bound = M.ssim_fast(a, b, g=g, rho=rho)
    assert abs(s - M.ssim(a, b)) <= bound * 1.01 + 1e-12
    fast, ref = M.ms_ssim_scales(a, b, g=g, rho=rho), M.ms_ssim_scales_def(a, b)
    for l in range(5):
        assert np.all(np.abs(fast[l][0] - ref[l]) <= fast[l][1] * 1.01 + 1e-12), (l, fast[l], ref[l])
    assert M.ms_ssim_from_scales(fast)[0] == pytest.approx(M.ms_ssim(a, b), abs=M.ms_ssim_from_scales(fast)[1] * 1.01 + 1e-12)


def test_fast_reference_geometry_rules():
    """piq 0.8.0's rules as the module docstring states them"""
    assert [M.grey_pool_factor(n, 5000) for n in (383, 384, 385, 639, 640, 641, 895, 896, 1152, 11)] == [1, 2, 2, 2, 2, 3, 3, 4, 4, 1]
    assert [M.grey_pool_factor(n, 5000, "half_up") for n in (384, 640, 896, 1152)] == [2, 3, 4, 5]
    a = np.zeros((163, 165, 3), np.float32)
    a[0, 0] = 1
    (v0, _), (v1, _) = M.ms_ssim_scales(a, a)[:2]
    assert np.allclose(v0, 1) and np.allclose(v1, 1)
    a = np.random.default_rng(0).random((30, 31, 3)).astype(np.float32)
    xa, _ = M.grey_planes(a, a)
    assert xa.shape == (30, 31)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def A():
    import adaptive_edge_aware_jpeg_amd as A
    return A


SIZES = [(176, 200), (175, 211), (161, 161), (300, 520), (384, 400), (600, 700), (640, 650)]      # f = 1, 1, 1, 1, 2 (1.5 -> 2), 2, 2 (2.5 -> 2)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_metrics_match_restatement(A, oracle, H, W):
    a, b = pair(oracle, H, W, H + W)
    m = A.EvaluationMetrics(A.Image.from_array(a), A.Image.from_array(b))
    assert float(m.psnr()) == pytest.approx(M.psnr(a, b), abs=PSNR_TOL)
    assert float(m.ssim()) == pytest.approx(M.ssim(a, b), abs=SSIM_TOL)
    assert float(m.ms_ssim()) == pytest.approx(M.ms_ssim(a, b), abs=SSIM_TOL)
    assert m.psnr().dtype == A._lib.get_context().torch.float32 and m.psnr().ndim == 0


@pytest.mark.gpu
def test_metrics_batch_and_round_trip(A, oracle):
    """What the sweep does (metrics_computation.py:168-190): compress -> decompress -> score, for a batch."""
    imgs = np.stack([oracle.synth_image(192, 256, s, k).astype(np.float32) / np.float32(255.0) for s, k in ((1, "mixed"), (2, "noise"), (3, "flat"))])
    codec = A.Jpeg(A.JpegCompressionSettings("YCbCr", (40, 80), (4, 64)))
    dec = codec.decompress_batch(codec.compress_batch(imgs))
    got = A.EvaluationMetrics.batch(imgs, dec).cpu().numpy()
    dec_h = dec.cpu().numpy()
    for i in range(len(imgs)):
        assert got[i, 0] == pytest.approx(M.psnr(imgs[i], dec_h[i]), abs=PSNR_TOL)
        assert got[i, 1] == pytest.approx(M.ssim(imgs[i], dec_h[i]), abs=SSIM_TOL)
        assert got[i, 2] == pytest.approx(M.ms_ssim(imgs[i], dec_h[i]), abs=SSIM_TOL)
    assert got[2, 0] > 40 and got[0, 0] > 25                                   # flat image survives almost untouched
    only = A.EvaluationMetrics.batch(imgs, dec, which=1).cpu().numpy()
    assert np.allclose(only[:, 0], got[:, 0]) and np.isnan(only[:, 1:]).all()


@pytest.mark.gpu
def test_metrics_identical_images_full_size(A, oracle):
    x = A._lib.get_context().torch.rand((1, 2160, 3840, 3), device="cuda")
    got = A.EvaluationMetrics.batch(x, x.clone()).cpu().numpy()[0]
    assert got[0] == pytest.approx(80.0, abs=1e-9) and got[1] == pytest.approx(1.0, abs=1e-6) and got[2] == pytest.approx(1.0, abs=1e-6)


@pytest.mark.gpu
def test_metrics_errors(A, oracle):
    a, b = pair(oracle, 100, 120, 1)
    m = A.EvaluationMetrics(A.Image.from_array(a), A.Image.from_array(b))
    assert float(m.psnr()) == pytest.approx(M.psnr(a, b), abs=PSNR_TOL)
    assert float(m.ssim()) == pytest.approx(M.ssim(a, b), abs=SSIM_TOL)
    with pytest.raises(ValueError):
        m.ms_ssim()                                                            # piq: "expected at least 161x161"
    with pytest.raises(ValueError):
        A.EvaluationMetrics(A.Image.from_array(a[:8]), A.Image.from_array(b[:8])).ssim()
    with pytest.raises(TypeError):
        A.EvaluationMetrics("a.png", "b.png").psnr()
    with pytest.raises(NotImplementedError):
        m.lpips()
