"""Evaluation path of the reference's ``InceptionMetrics`` callback (core/callback_inception_metrics.py:136-246;
SURVEY.md 8-f3) minus the Inception network itself, whose weights are fetched from a URL
(core/submodules/gan_stability/metrics/inception.py:13) and cannot be obtained offline:

* ``SampleDump``   -- the fixed latent set drawn once from the HOST generator at construction (:166-168) and the
                      eval-mode generator sweep over it on the GPU (:183-203), producing the same uint8 HWC images
                      the callback writes to PNG files (including its clamp of the tanh output to [0, 1]);
* ``activation_statistics`` / ``frechet_distance`` -- FID from two activation sets (:223-231; the formula of
                      core/submodules/gan_stability/metrics/fid_score.py:25-80);
* ``polynomial_mmd_averages`` -- KID (:15-133, :233-234).

``evaluate`` strings them together around any ``feature_fn(images_uint8_nhwc) -> [n, d]`` feature extractor.
The arithmetic is pinned to the reference's own functions by tests/golden/eval_metrics.npz
(tests/golden/make_eval_golden.py).  Host-side numpy / scipy like the reference; only the generator runs on the GPU -- and, opt-in
(``kid_on_device``), KID's kernel-matrix sums (``polynomial_mmd_averages_device``, csrc/gz_kid.hip).

``evaluate_device`` is the same evaluation with the activations resident on the GPU from the generator to the two small
results that leave it: ``SampleDump.device_batches`` (generator output -> Inception input in one launch,
gz_samples_to_inception_input), the network at a large batch, fp64 mean / covariance (``feature_moments_device``,
csrc/gz_moments.hip) and KID's sums.  The matrix square root stays on the host unless ``fid_on_device`` asks for
``frechet_distance_device``: two Newton-Schulz square roots of symmetric positive semi-definite matrices, matrix products
alone, on the fp64 MFMA product of csrc/gz_sqrtm.hip.  ``frechet_distance_newton_schulz`` is the same recurrence in numpy.
With ``classifier=`` it also reports the Inception Score (gan_stability's metrics/inception_score.py) of the resident
codes: ``inception_score_device`` on csrc/gz_inception_score.hip, ``inception_score_from_logits`` its host yardstick.
With ``prdc_k=`` it reports improved precision / recall and density / coverage of the two resident code sets as well:
``prdc_device`` on csrc/gz_prdc.hip, ``prdc`` its host yardstick (the reference has neither).

``evaluate_swd`` is a metric that needs none of that -- no network, no weight file: the sliced Wasserstein distance on
Laplacian-pyramid patches (Karras et al. 2018), one number per resolution level, from the pixels of a real and a generated
set alone.  ``swd`` (with ``laplacian_pyramid``, ``swd_descriptors``, ``sliced_wasserstein``) is its definition in numpy
fp64, ``swd_device`` the same statistic on csrc/gz_swd.hip, ``SwdPlan`` its draws, ``RealPyramid`` the real set's resident
side (the reference has no such metric).
"""
import numpy as np
import torch


class SampleDump:
    def __init__(self, module, n_samples=5000, batch_size=16):
        # drawn from the host generator right after the module is built, like the callback's __init__ (:166-168)
        self.n_samples, self.batch_size = n_samples, batch_size
        self.z_samples = torch.split(module.noise_distn.sample((n_samples, module.cfg.model.noise_dim)), batch_size)

    @torch.no_grad()
    def images(self, module):
        """Yields uint8 arrays [b, H, W, 3]: generator in eval mode over the fixed latents (:186-198)."""
        was_training = module.training
        module.eval()
        try:
            for z in self.z_samples:
                samples = module.generator(z.to(module.device))
                if samples.shape[1] == 1:                     # greyscale -> RGB (:193-195)
                    samples = torch.cat(3 * [samples], dim=1)
                samples = torch.clamp(samples, 0, 1)          # sic: the tanh output is clamped, not de-normalised (:197)
                samples = samples.permute(0, 2, 3, 1).detach().cpu().numpy()
                yield (samples * 255).astype(int).astype(np.uint8)
        finally:
            module.train(was_training)

    @torch.no_grad()
    def device_batches(self, module, batch=250, size=(299, 299), mul=2.0, add=-1.0):
        """Yields float32 device tensors [b, 3, size[0], size[1]]: the images of ``images`` as InceptionV3 reads them --
        clamp, grey level, ToTensor, bilinear resize, ``* mul + add`` -- made from the generator's output by one launch
        (gz_samples_to_inception_input), bit-equal to ``images`` -> ``functional.normalize_u8_images(u8, 0, 1)`` ->
        gz_resize_bilinear.  Eval mode under no_grad, mode restored afterwards.  A generator that draws on the host in
        every call (``sample_view``: HoloGAN's view, from numpy's global generator) is called on the dump's own splits,
        so numpy's stream is left exactly as ``images`` leaves it; any other generator is called on ``batch`` latents
        at a time.  No CPU fallback."""
        from . import functional as F
        from ._lib import check, lib
        if torch.device(module.device).type != "cuda":
            raise RuntimeError("lightning_gan_zoo_amd.eval: the device evaluation pass runs on the HIP kernels; device %r "
                               "is not a GPU and there is no fallback (use SampleDump.images)" % (module.device,))
        OH, OW = int(size[0]), int(size[1])
        if hasattr(module.generator, "sample_view"):
            splits = self.z_samples
        else:
            splits = torch.split(torch.cat(list(self.z_samples)), int(batch))
        was_training = module.training
        module.eval()
        try:
            for z in splits:
                samples = F._req(module.generator(z.to(module.device)).detach().float(), "samples")
                N, C, H, W = samples.shape
                y = torch.empty((N, 3, OH, OW), device=samples.device, dtype=torch.float32)
                with torch.cuda.device(samples.device):
                    check(lib.gz_samples_to_inception_input(F._p(samples), F._p(y), N, C, H, W, OH, OW, float(mul),
                                                            float(add), F._stream()), "samples_to_inception_input")
                yield y
        finally:
            module.train(was_training)


def make_grid(images, nrow=8, padding=2, normalize=False, pad_value=0.0):
    """torchvision.utils.make_grid for a [N, C, H, W] tensor (the subset the reference uses,
    core/lightning_module.py:68-69: ``normalize=True``, defaults otherwise): with ``normalize`` the WHOLE tensor is
    shifted / scaled to [0, 1] by its own min / max (``scale_each=False``, the 1e-5 guard of torchvision's
    ``norm_ip``); images are laid out ``nrow`` per row with ``padding`` pixels of ``pad_value`` around each;
    single-channel input is repeated to three channels."""
    t = images.detach()
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.shape[1] == 1:
        t = torch.cat((t, t, t), 1)
    if normalize:
        t = t.clone()
        lo, hi = float(t.min()), float(t.max())
        t = t.clamp(min=lo, max=hi).sub(lo).div(max(hi - lo, 1e-5))
    n = t.shape[0]
    if n == 1:
        return t.squeeze(0)
    xmaps = min(nrow, n)
    ymaps = int(np.ceil(float(n) / xmaps))
    height, width = int(t.shape[2] + padding), int(t.shape[3] + padding)
    grid = t.new_full((t.shape[1], height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= n:
                break
            grid[:, y * height + padding:(y + 1) * height, x * width + padding:(x + 1) * width] = t[k]
            k += 1
    return grid


def activation_statistics(act):
    act = np.asarray(act)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = |mu1 - mu2|^2 + Tr(S1 + S2 - 2 (S1 S2)^(1/2)); returns nan when the matrix square root has a
    non-negligible imaginary diagonal (fid_score.py:25-80)."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape:
        raise ValueError("the two statistics have different dimensions")
    delta = mu1 - mu2
    root, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(root).all():          # nearly singular product: regularise both covariances
        ridge = np.eye(sigma1.shape[0]) * eps
        root = linalg.sqrtm((sigma1 + ridge).dot(sigma2 + ridge))
    if np.iscomplexobj(root):
        if not np.allclose(np.diagonal(root).imag, 0, atol=1e-3):
            return float("nan")
        root = root.real
    return float(delta.dot(delta) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(root))


NS_MAXIT = 100          # iterations after which a Newton-Schulz root counts as not converged
NS_TOL = 1e-14          # the trace moved by no more than this, relatively: converged
NS_FLOOR = 1e-10        # the trace's movement stopped shrinking below this: the rounding floor, keep the iterate before


def _ns_verdict(t, tn, dprev):
    """The stop rule of the coupled Newton-Schulz iteration from the traces of two successive iterates ->
    (verdict, |tn - t|): "fail" (not finite), "new" (converged, take the new iterate), "old" (the rounding floor is
    reached: on a rank-deficient matrix the noise in the null space grows from here on, take the iterate before) or
    "go".  One function for the numpy restatement and the device loop."""
    dk = abs(tn - t)
    if not np.isfinite(tn):
        return "fail", dk
    if dk <= NS_TOL * abs(tn):
        return "new", dk
    if dk >= dprev and dk <= NS_FLOOR * abs(tn):
        return "old", dk
    return "go", dk


def _newton_schulz(a, maxit=NS_MAXIT):
    """Coupled Newton-Schulz iteration for the square root of a symmetric positive semi-definite matrix, plain products,
    nothing symmetrised: Y0 = A / c, Z0 = I, T = 1.5 I - 0.5 Z Y, Y <- Y T, Z <- T Z with c = |A|_F, so that
    sqrt(A) ~ sqrt(c) Y.  -> (Y, c, trace(Y), iterations, converged)."""
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    d = a.shape[0]
    c = float(np.sqrt(np.sum(a * a)))
    if c == 0.0:
        return np.zeros_like(a), 0.0, 0.0, 0, True
    if not np.isfinite(c):
        return a, c, float("nan"), 0, False
    eye = np.eye(d)
    y, z = a / c, eye.copy()
    t, dprev = float(np.trace(y)), float("inf")
    for k in range(1, int(maxit) + 1):
        tk = 1.5 * eye - 0.5 * z.dot(y)
        yn, z = y.dot(tk), tk.dot(z)
        tn = float(np.trace(yn))
        verdict, dk = _ns_verdict(t, tn, dprev)
        if verdict == "fail":
            return y, c, t, k, False
        if verdict == "new":
            return yn, c, tn, k, True
        if verdict == "old":
            return y, c, t, k, True
        y, t, dprev = yn, tn, dk
    return y, c, t, int(maxit), False


def sqrtm_psd_newton_schulz(a, maxit=NS_MAXIT):
    """-> (root, iterations, converged) of a symmetric positive semi-definite matrix (``_newton_schulz``)."""
    y, c, _, k, ok = _newton_schulz(a, maxit)
    return np.sqrt(c) * y, k, ok


def frechet_distance_newton_schulz(mu1, sigma1, mu2, sigma2, maxit=NS_MAXIT):
    """The Frechet distance with Tr (S1 S2)^(1/2) = Tr (R S2 R)^(1/2), R = S1^(1/2): two roots of symmetric positive
    semi-definite matrices by ``_newton_schulz``.  The CPU restatement of ``frechet_distance_device``.
    -> (distance, (iterations of R, iterations of the second root), converged: both did)."""
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape:
        raise ValueError("the two statistics have different dimensions")
    delta = mu1 - mu2
    root1, k1, ok1 = sqrtm_psd_newton_schulz(sigma1, maxit)
    _, c, t, k2, ok2 = _newton_schulz(root1.dot(sigma2).dot(root1), maxit)
    fid = float(delta.dot(delta) + np.trace(sigma1) + np.trace(sigma2) - 2 * (np.sqrt(c) * t))
    return fid, (k1, k2), bool(ok1 and ok2)


def _poly_kernel(x, y, degree, gamma, coef0):
    if gamma is None:
        gamma = 1.0 / x.shape[1]
    return (gamma * x.dot(y.T) + coef0) ** degree


def _sq(a):
    a = np.ravel(a)
    return a.dot(a)


def _mmd2(m, sx, sy, sxy):
    """The unbiased MMD^2 estimate from the sums of K_xx and K_yy without their diagonals and the sum of K_xy; scalars
    (one subset) or [S] arrays."""
    return (sx + sy) / (m * (m - 1)) - 2 * sxy / (m * m)


def _mmd2_variance(m, var_at_m, sx, sy, sxy, sx2, sy2, sxy2, dxx, dyy, rx2, ry2, cxy1_2, cxy0_2):
    """The estimator's variance estimate (callback_inception_metrics.py:57-133) from reduced quantities, scalars or [S]
    arrays: ``s*`` the sums of ``_mmd2``, ``s*2`` the sums of squared entries (diagonals excluded for xx, yy),
    ``dxx = <rx, cxy1>``, ``dyy = <ry, cxy0>`` and the squared norms of the row sums rx, ry (without diagonal) and of
    K_xy's row sums cxy1 and column sums cxy0.  The callers make the reductions; the expressions exist once."""
    m1, m2 = m - 1, m - 2
    zeta1 = (1 / (m * m1 * m2) * (rx2 - sx2 + ry2 - sy2)
             - 1 / (m * m1) ** 2 * (sx ** 2 + sy ** 2)
             + 1 / (m * m * m1) * (cxy1_2 + cxy0_2 - 2 * sxy2)
             - 2 / m ** 4 * sxy ** 2
             - 2 / (m * m * m1) * (dxx + dyy)
             + 2 / (m ** 3 * m1) * (sx + sy) * sxy)
    zeta2 = (1 / (m * m1) * (sx2 + sy2)
             - 1 / (m * m1) ** 2 * (sx ** 2 + sy ** 2)
             + 2 / (m * m) * sxy2
             - 2 / m ** 4 * sxy ** 2
             - 4 / (m * m * m1) * (dxx + dyy)
             + 4 / (m ** 3 * m1) * (sx + sy) * sxy)
    return 4 * (var_at_m - 2) / (var_at_m * (var_at_m - 1)) * zeta1 + 2 / (var_at_m * (var_at_m - 1)) * zeta2


def _mmd2_and_variance(k_xx, k_xy, k_yy, var_at_m=None, ret_var=True):
    """Unbiased MMD^2 estimate and its variance estimate from three m x m kernel matrices
    (callback_inception_metrics.py:57-133, the 'unbiased' estimator with explicit diagonals)."""
    m = k_xx.shape[0]
    if var_at_m is None:
        var_at_m = m
    dx, dy = np.diagonal(k_xx), np.diagonal(k_yy)
    rx = k_xx.sum(axis=1) - dx              # row sums without the diagonal
    ry = k_yy.sum(axis=1) - dy
    cxy0, cxy1 = k_xy.sum(axis=0), k_xy.sum(axis=1)
    sx, sy, sxy = rx.sum(), ry.sum(), cxy0.sum()
    mmd2 = _mmd2(m, sx, sy, sxy)
    if not ret_var:
        return mmd2
    sx2 = _sq(k_xx) - _sq(dx)
    sy2 = _sq(k_yy) - _sq(dy)
    sxy2 = _sq(k_xy)
    dxx = rx.dot(cxy1)
    dyy = ry.dot(cxy0)
    return mmd2, _mmd2_variance(m, var_at_m, sx, sy, sxy, sx2, sy2, sxy2, dxx, dyy, _sq(rx), _sq(ry), _sq(cxy1),
                                _sq(cxy0))


def polynomial_mmd(codes_g, codes_r, degree=3, gamma=None, coef0=1, var_at_m=None, ret_var=True):
    """k(x, y) = (gamma <x, y> + coef0)^degree, gamma = 1 / dim by default (:42-55)."""
    k_xx = _poly_kernel(codes_g, codes_g, degree, gamma, coef0)
    k_yy = _poly_kernel(codes_r, codes_r, degree, gamma, coef0)
    k_xy = _poly_kernel(codes_g, codes_r, degree, gamma, coef0)
    return _mmd2_and_variance(k_xx, k_xy, k_yy, var_at_m=var_at_m, ret_var=ret_var)


def polynomial_mmd_averages(codes_g, codes_r, n_subsets=50, subset_size=1000, ret_var=True, **kernel_args):
    """KID: MMD^2 over ``n_subsets`` random subsets drawn with numpy's GLOBAL generator, without replacement, the
    generated codes first (:19-40).  Note the callback passes (real_act, fake_act) in that order (:233)."""
    subset_size = min(len(codes_g), len(codes_r), subset_size)
    m = min(codes_g.shape[0], codes_r.shape[0])
    mmds = np.zeros(n_subsets)
    variances = np.zeros(n_subsets)
    for i in range(n_subsets):
        g = codes_g[np.random.choice(len(codes_g), subset_size, replace=False)]
        r = codes_r[np.random.choice(len(codes_r), subset_size, replace=False)]
        o = polynomial_mmd(g, r, **kernel_args, var_at_m=m, ret_var=ret_var)
        if ret_var:
            mmds[i], variances[i] = o
        else:
            mmds[i] = o
    return (mmds, variances) if ret_var else mmds


def _mmd2_and_variance_from_sums(sums, m, var_at_m=None, ret_var=True):
    """``_mmd2_and_variance`` for S subsets at once, from the ``6 m + 3`` numbers per subset that gz_kid_sums writes
    (include/gz_ops.h): rowsum(K_xx) with the diagonal | diag(K_xx) | rowsum(K_yy) | diag(K_yy) | rowsum(K_xy) |
    colsum(K_xy) | the three squared Frobenius norms -- all the estimator reads of the matrices.  ``sums``: [S, 6m+3]."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 2 or sums.shape[1] != 6 * m + 3:
        raise ValueError("expected [S, %d] sums for m = %d, got %s" % (6 * m + 3, m, sums.shape))
    if var_at_m is None:
        var_at_m = m
    dx, dy = sums[:, m:2 * m], sums[:, 3 * m:4 * m]
    rx = sums[:, :m] - dx                   # row sums without the diagonal
    ry = sums[:, 2 * m:3 * m] - dy
    cxy1, cxy0 = sums[:, 4 * m:5 * m], sums[:, 5 * m:6 * m]
    sx, sy, sxy = rx.sum(axis=1), ry.sum(axis=1), cxy0.sum(axis=1)
    mmd2 = _mmd2(m, sx, sy, sxy)
    if not ret_var:
        return mmd2

    def sq(a):
        return np.einsum("sm,sm->s", a, a)

    sx2 = sums[:, 6 * m] - sq(dx)
    sy2 = sums[:, 6 * m + 1] - sq(dy)
    sxy2 = sums[:, 6 * m + 2]
    dxx = np.einsum("sm,sm->s", rx, cxy1)
    dyy = np.einsum("sm,sm->s", ry, cxy0)
    return mmd2, _mmd2_variance(m, var_at_m, sx, sy, sxy, sx2, sy2, sxy2, dxx, dyy, sq(rx), sq(ry), sq(cxy1),
                                sq(cxy0))


def draw_kid_subsets(n_g, n_r, n_subsets, subset_size):
    """The rows ``polynomial_mmd_averages`` would pick: the same ``np.random.choice(..., replace=False)`` calls on
    numpy's GLOBAL generator in the same order (g then r, subset after subset), so the generator is left in the state
    the host loop leaves it in.  ``subset_size`` is clamped like there.  -> int32 [n_subsets, 2, m]."""
    m = min(n_g, n_r, subset_size)
    idx = np.empty((n_subsets, 2, m), dtype=np.int32)
    for i in range(n_subsets):
        idx[i, 0] = np.random.choice(n_g, m, replace=False)
        idx[i, 1] = np.random.choice(n_r, m, replace=False)
    return idx


def device_codes(codes, device):
    """[n, d] codes as a contiguous fp64 tensor on ``device`` (fp32 is widened there: exact)."""
    t = codes if isinstance(codes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(codes))
    if t.dim() != 2 or not (t.dtype.is_floating_point or t.dtype in (torch.int32, torch.int64)):
        raise ValueError("codes must be a real [n, d] array, got %s %s" % (t.dtype, tuple(t.shape)))
    t = t.detach().to(device).to(torch.float64).contiguous()
    if not t.is_cuda:
        raise RuntimeError("lightning_gan_zoo_amd.eval: the device KID path runs on the HIP kernels; device %r is not a "
                           "GPU and there is no fallback (use polynomial_mmd_averages)" % (device,))
    return t


def kid_sums_device(codes_g, codes_r, idx, degree=3, gamma=None, coef0=1):
    """gz_kid_sums (csrc/gz_kid.hip) on fp64 device codes for the host index table ``idx`` [S, 2, m] (checked here: the
    kernel trusts it).  One upload of the indices, two launches, one copy back.  -> numpy [S, 6m+3]."""
    from . import functional as F
    from ._lib import check, lib
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    if idx.ndim != 3 or idx.shape[1] != 2 or idx.size == 0:
        raise ValueError("idx must be a non-empty [S, 2, m] table, got %s" % (idx.shape,))
    S, _, m = idx.shape
    (n_g, d), n_r = codes_g.shape, codes_r.shape[0]
    if codes_r.shape[1] != d:
        raise ValueError("the two code sets have different dimensions (%d, %d)" % (d, codes_r.shape[1]))
    if idx.min() < 0 or idx[:, 0].max() >= n_g or idx[:, 1].max() >= n_r:
        raise ValueError("subset rows outside the code sets")
    if gamma is None:
        gamma = 1.0 / d
    with torch.cuda.device(codes_g.device):
        idx_dev = torch.from_numpy(idx).to(codes_g.device)
        out = torch.empty((S, 6 * m + 3), dtype=torch.float64, device=codes_g.device)
        ws_bytes = lib.gz_kid_workspace_bytes(S, m, d)
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=codes_g.device)
        check(lib.gz_kid_sums(F._p(codes_g), n_g, F._p(codes_r), n_r, d, F._p(idx_dev), S, m, float(gamma), float(coef0),
                              int(degree), F._p(out), F._p(ws), ws_bytes, F._stream()), "kid_sums")
        return out.cpu().numpy()


def polynomial_mmd_averages_device(codes_g, codes_r, n_subsets=50, subset_size=1000, ret_var=True, degree=3, gamma=None,
                                   coef0=1, device="cuda"):
    """``polynomial_mmd_averages`` with the kernel matrices' sums computed on the GPU (csrc/gz_kid.hip, fp64 MFMA): the
    same subsets from numpy's global generator, left in the same state; the same values up to the order of fp64
    summation.  ``codes_*``: numpy arrays or torch tensors (tensors already on the device in fp64 are used as they
    are); the estimator's O(S m) formula runs on the host."""
    g, r = device_codes(codes_g, device), device_codes(codes_r, device)
    if r.device != g.device:
        r = r.to(g.device)
    idx = draw_kid_subsets(g.shape[0], r.shape[0], n_subsets, subset_size)
    sums = kid_sums_device(g, r, idx, degree=degree, gamma=gamma, coef0=coef0)
    return _mmd2_and_variance_from_sums(sums, idx.shape[2], var_at_m=min(g.shape[0], r.shape[0]), ret_var=ret_var)


def feature_moments_device(codes):
    """(mean [d], cov [d, d]) of fp64 device codes [n, d] as fp64 device tensors: ``np.mean(codes, axis=0)`` and
    ``np.cov(codes, rowvar=False)`` in numpy's two-pass form on the fp64 MFMA kernel (gz_feature_moments,
    csrc/gz_moments.hip).  Deterministic, cov bitwise symmetric.  No CPU fallback."""
    from . import functional as F
    from ._lib import check, lib
    if not isinstance(codes, torch.Tensor) or codes.dim() != 2 or codes.dtype != torch.float64:
        raise ValueError("codes must be a float64 [n, d] tensor (eval.device_codes makes one)")
    if not codes.is_cuda:
        raise RuntimeError("lightning_gan_zoo_amd.eval: the device moments run on the HIP kernels; device %r is not a GPU "
                           "and there is no fallback (use activation_statistics)" % (codes.device,))
    codes = codes if codes.is_contiguous() else codes.contiguous()
    n, d = codes.shape
    with torch.cuda.device(codes.device):
        mean = torch.empty((d,), dtype=torch.float64, device=codes.device)
        cov = torch.empty((d, d), dtype=torch.float64, device=codes.device)
        ws_bytes = lib.gz_feature_moments_workspace_bytes(n, d)
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=codes.device)
        check(lib.gz_feature_moments(F._p(codes), n, d, F._p(mean), F._p(cov), F._p(ws), ws_bytes, F._stream()),
              "feature_moments")
    return mean, cov


def inception_score_from_logits(logits, splits=10):
    """Inception Score of classifier logits [n, classes] on the host in numpy fp64 -> (mean, std, split_scores): the loop
    of the reference's core/submodules/gan_stability/metrics/inception_score.py:54-66 -- softmax over all classes,
    contiguous splits of ``n // splits`` rows (the trailing ``n % splits`` rows are ignored), ``scipy.stats.entropy(p_i,
    p_y)`` per row, ``exp(mean)`` per split, then mean and std over the splits.  The yardstick ``inception_score_device``
    is measured against.

    One deliberate difference from the reference lies in front of this function, not in it: the reference runs
    torchvision's ImageNet InceptionV3 (1000 classes) over the images a second time; here the logits come from the
    classifier head that the FID weight file carries (``FIDInceptionV3.fc``, 1008 classes of the 2015 network -- the one
    the score was defined on) applied to the pool features the evaluation already holds."""
    from scipy.stats import entropy
    logits = np.asarray(logits, dtype=np.float64)
    splits = int(splits)
    if logits.ndim != 2 or splits < 1 or splits > logits.shape[0]:
        raise ValueError("expected [n, classes] logits and 1 <= splits <= n, got %s and %d" % (logits.shape, splits))
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    preds = e / e.sum(axis=1, keepdims=True)
    m = logits.shape[0] // splits
    split_scores = []
    for k in range(splits):
        part = preds[k * m:(k + 1) * m]
        py = np.mean(part, axis=0)
        split_scores.append(np.exp(np.mean([entropy(part[i], py) for i in range(part.shape[0])])))
    split_scores = np.asarray(split_scores)
    return float(np.mean(split_scores)), float(np.std(split_scores)), split_scores


def _fp64_device_codes(codes, what, instead):
    if not isinstance(codes, torch.Tensor) or codes.dim() != 2 or codes.dtype != torch.float64:
        raise ValueError("codes must be a float64 [n, d] tensor (eval.device_codes makes one)")
    if not codes.is_cuda:
        raise RuntimeError("lightning_gan_zoo_amd.eval: the device %s runs on the HIP kernels; device %r is not a GPU "
                           "and there is no fallback (use %s)" % (what, codes.device, instead))
    return codes if codes.is_contiguous() else codes.contiguous()


def _classifier_on(device, weight, bias, d):
    """(weight [classes, d], bias [classes] or None) as contiguous fp64 tensors on ``device`` (fp32 is widened: exact)."""
    def fp64(t):
        t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.array(t))
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError("the classifier's weight and bias must be float32 or float64, got %s" % t.dtype)
        return t.detach().to(device).to(torch.float64).contiguous()
    weight = fp64(weight)
    if weight.dim() != 2 or weight.shape[1] != d:
        raise ValueError("weight must be [classes, %d] (nn.Linear's layout), got %s" % (d, tuple(weight.shape)))
    if bias is not None:
        bias = fp64(bias)
        if tuple(bias.shape) != (weight.shape[0],):
            raise ValueError("bias must be [%d], got %s" % (weight.shape[0], tuple(bias.shape)))
    return weight, bias


def classifier_logits_device(codes, weight, bias=None):
    """``codes @ weight.T + bias`` for fp64 device codes [n, d] as an fp64 device tensor [n, classes], on the fp64 MFMA
    kernel (gz_classifier_logits, csrc/gz_inception_score.hip).  ``weight`` [classes, d] / ``bias`` [classes]: the
    classifier head of the FID weight file (``FIDInceptionV3.fc`` -- not torchvision's ImageNet network, see
    ``inception_score_from_logits``), float32 or float64 on any device, converted once.  No CPU fallback."""
    from . import functional as F
    from ._lib import check, lib
    codes = _fp64_device_codes(codes, "classifier logits", "numpy's dot")
    n, d = codes.shape
    weight, bias = _classifier_on(codes.device, weight, bias, d)
    classes = weight.shape[0]
    with torch.cuda.device(codes.device):
        logits = torch.empty((n, classes), dtype=torch.float64, device=codes.device)
        check(lib.gz_classifier_logits(F._p(codes), n, d, F._p(weight), None if bias is None else F._p(bias), classes,
                                       F._p(logits), F._stream()), "classifier_logits")
    return logits


def inception_score_device(codes, weight, bias=None, splits=10):
    """``inception_score_from_logits(codes @ weight.T + bias, splits)`` on the device -> (mean, std, split_scores) as
    floats and a numpy array: two C-ABI calls (gz_classifier_logits, gz_inception_score; csrc/gz_inception_score.hip),
    the ``splits`` doubles copied back, their mean and std taken on the host.  The classifier is the head of the FID
    weight file, not the reference's torchvision network (``inception_score_from_logits``).  No CPU fallback."""
    from . import functional as F
    from ._lib import check, lib
    logits = classifier_logits_device(codes, weight, bias)
    (n, classes), splits = logits.shape, int(splits)
    if splits < 1 or splits > n:
        raise ValueError("splits must lie in 1 .. n = %d, got %d" % (n, splits))
    with torch.cuda.device(logits.device):
        scores = torch.empty((splits,), dtype=torch.float64, device=logits.device)
        ws_bytes = lib.gz_inception_score_workspace_bytes(n, classes, splits)
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=logits.device)
        check(lib.gz_inception_score(F._p(logits), n, classes, splits, F._p(scores), F._p(ws), ws_bytes, F._stream()),
              "inception_score")
        split_scores = scores.cpu().numpy()
    return float(np.mean(split_scores)), float(np.std(split_scores)), split_scores


PRDC_MAX_K = 8          # the device kernels keep a row's k smallest distances in registers (csrc/gz_prdc.hip)


def _prdc_check(k, *sets):
    k = int(k)
    d = None
    for codes in sets:
        if codes.ndim != 2 or codes.shape[1] < 1 or (d is not None and codes.shape[1] != d):
            raise ValueError("codes must be [n, d] arrays of one d >= 1, got %s" % (tuple(codes.shape),))
        d = codes.shape[1]
    if k < 1 or k > PRDC_MAX_K or k >= min(c.shape[0] for c in sets):
        raise ValueError("k must lie in 1 .. %d and below the smaller set's %d rows, got %d"
                         % (PRDC_MAX_K, min(c.shape[0] for c in sets), k))
    return k


def _sq_distances(x, y):
    """Squared Euclidean distances [len(x), len(y)] from direct differences, ``((x_i - y_j) ** 2).sum()``."""
    return ((x[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)


def _row_blocks(n, n_other, d, budget=1 << 21):
    """Row ranges whose [rows, n_other, d] difference block stays under ``budget`` doubles."""
    step = max(1, int(budget // max(1, n_other * d)))
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def knn_radii(codes, k):
    """``rad[i]``: the k-th smallest SQUARED distance from row i to the other rows of ``codes`` [n, d], self excluded by
    index (exact duplicates give 0).  Numpy fp64 on direct differences, blocked over rows.  The yardstick of
    ``knn_radii_device``."""
    codes = np.asarray(codes, dtype=np.float64)
    k = _prdc_check(k, codes)
    n, d = codes.shape
    rad = np.empty(n)
    for a, b in _row_blocks(n, n, d):
        dist = _sq_distances(codes[a:b], codes)
        dist[np.arange(b - a), np.arange(a, b)] = np.inf
        rad[a:b] = np.partition(dist, k - 1, axis=1)[:, k - 1]
    return rad


def prdc(codes_g, codes_r, k=5):
    """Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) of generated
    codes ``codes_g`` [n_g, d] against real codes ``codes_r`` [n_r, d] on the host: numpy fp64 on SQUARED distances from
    direct differences (deliberately not the Gram form the device uses), blocked over rows.  With ``rad_X[i]`` the k-th
    smallest distance from row i of X to the other rows of X (``knn_radii``):

        in_real[j] = #{i : D(G_j, R_i) <= rad_R[i]}      in_fake[i] = #{j : D(G_j, R_i) <= rad_G[j]}
        near[i]    = min_j D(G_j, R_i)
        precision  = #{in_real > 0} / n_g                recall   = #{in_fake > 0} / n_r
        density    = sum in_real / (k n_g)               coverage = #{near <= rad_R} / n_r

    Every comparison is ``<=``, as in the improved precision and recall paper.  The ``prdc`` package of the density and
    coverage paper is remembered to compare with a strict ``<``, which differs on exact ties only; neither package was
    at hand to check, so that is a recollection, not a verified fact.  ``k`` = 5 is the density and coverage paper's
    value (Kynkaanniemi et al. use 3).  -> dict of the four floats, the per-row arrays ``in_real`` [n_g], ``in_fake``
    [n_r], ``near`` [n_r] and the radii ``rad_g``, ``rad_r``.  The yardstick ``prdc_device`` is measured against."""
    g, r = np.asarray(codes_g, dtype=np.float64), np.asarray(codes_r, dtype=np.float64)
    k = _prdc_check(k, g, r)
    (n_g, d), n_r = g.shape, r.shape[0]
    rad_g, rad_r = knn_radii(g, k), knn_radii(r, k)
    in_real = np.empty(n_g, dtype=np.int64)
    in_fake = np.zeros(n_r, dtype=np.int64)
    near = np.full(n_r, np.inf)
    for a, b in _row_blocks(n_g, n_r, d):
        dist = _sq_distances(g[a:b], r)
        in_real[a:b] = (dist <= rad_r[None, :]).sum(axis=1)
        in_fake += (dist <= rad_g[a:b, None]).sum(axis=0)
        near = np.minimum(near, dist.min(axis=0))
    return {"precision": float((in_real > 0).sum() / n_g), "recall": float((in_fake > 0).sum() / n_r),
            "density": float(in_real.sum() / (k * n_g)), "coverage": float((near <= rad_r).sum() / n_r),
            "in_real": in_real, "in_fake": in_fake, "near": near, "rad_g": rad_g, "rad_r": rad_r}


def knn_radii_device(codes, k):
    """``knn_radii`` of fp64 device codes [n, d] as an fp64 device tensor [n]: gz_knn_radii (csrc/gz_prdc.hip), squared
    distances in the Gram form on the fp64 MFMA tile core.  Bit-deterministic.  No CPU fallback."""
    from . import functional as F
    from ._lib import check, lib
    codes = _fp64_device_codes(codes, "k-nearest-neighbour radii", "eval.knn_radii")
    k = _prdc_check(k, codes)
    n, d = codes.shape
    with torch.cuda.device(codes.device):
        radii = torch.empty((n,), dtype=torch.float64, device=codes.device)
        ws_bytes = lib.gz_knn_radii_workspace_bytes(n, d, k)
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=codes.device)
        check(lib.gz_knn_radii(F._p(codes), n, d, k, F._p(radii), F._p(ws), ws_bytes, F._stream()), "knn_radii")
    return radii


def prdc_device(codes_g, codes_r, k=5, rad_r=None, rad_g=None):
    """``prdc`` on fp64 device codes: two gz_knn_radii calls and one gz_prdc_counts walk over the cross distances
    (csrc/gz_prdc.hip); the 32 bytes of integer totals are all that travels to the host, where the four quotients are
    taken.  ``rad_r`` / ``rad_g``: radii already known as fp64 device tensors (``RealStatistics.radii`` keeps the real
    set's).  -> the same keys as ``prdc``: four floats, and ``in_real`` / ``in_fake`` (int32), ``near``, ``rad_g``,
    ``rad_r`` as device tensors.  No CPU fallback."""
    from . import functional as F
    from ._lib import check, lib
    g = _fp64_device_codes(codes_g, "precision / recall / density / coverage", "eval.prdc")
    r = _fp64_device_codes(codes_r, "precision / recall / density / coverage", "eval.prdc")
    if r.device != g.device:
        raise ValueError("the two code sets lie on different devices (%s, %s)" % (g.device, r.device))
    k = _prdc_check(k, g, r)
    (n_g, d), n_r = g.shape, r.shape[0]

    def radii(given, codes):
        if given is None:
            return knn_radii_device(codes, k)
        if (not isinstance(given, torch.Tensor) or given.dtype != torch.float64 or given.device != codes.device
                or tuple(given.shape) != (codes.shape[0],)):
            raise ValueError("radii must be a float64 [%d] tensor on %s" % (codes.shape[0], codes.device))
        return given.contiguous()

    rad_g, rad_r = radii(rad_g, g), radii(rad_r, r)
    with torch.cuda.device(g.device):
        in_real = torch.empty((n_g,), dtype=torch.int32, device=g.device)
        in_fake = torch.empty((n_r,), dtype=torch.int32, device=g.device)
        near = torch.empty((n_r,), dtype=torch.float64, device=g.device)
        totals = torch.empty((4,), dtype=torch.int64, device=g.device)
        ws_bytes = lib.gz_prdc_counts_workspace_bytes(n_g, n_r, d)
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=g.device)
        check(lib.gz_prdc_counts(F._p(g), n_g, F._p(rad_g), F._p(r), n_r, F._p(rad_r), d, F._p(in_real), F._p(in_fake),
                                 F._p(near), F._p(totals), F._p(ws), ws_bytes, F._stream()), "prdc_counts")
        precise, recalled, inside, covered = totals.tolist()
    return {"precision": precise / n_g, "recall": recalled / n_r, "density": inside / (k * n_g),
            "coverage": covered / n_r, "in_real": in_real, "in_fake": in_fake, "near": near, "rad_g": rad_g,
            "rad_r": rad_r}


def _square_fp64_device(a, what):
    if not isinstance(a, torch.Tensor) or a.dim() != 2 or a.shape[0] != a.shape[1] or a.dtype != torch.float64:
        raise ValueError("%s must be a square float64 tensor" % what)
    if not a.is_cuda:
        raise RuntimeError("lightning_gan_zoo_amd.eval: the device square root runs on the HIP kernels; device %r is not a "
                           "GPU and there is no fallback (use frechet_distance)" % (a.device,))
    return a if a.is_contiguous() else a.contiguous()


class _SqrtmLaunchers:
    """The launchers of csrc/gz_sqrtm.hip for d x d matrices on one device, with the reduction's workspace and its two
    result doubles allocated once."""

    def __init__(self, d, device):
        from . import functional as F
        from ._lib import check, lib
        self.F, self.check, self.lib, self.d = F, check, lib, int(d)
        self.ws_bytes = lib.gz_sqrtm_trace_norm_workspace_bytes(self.d)
        self.ws = torch.empty(max(self.ws_bytes, 8), dtype=torch.uint8, device=device)
        self.stats = torch.empty(2, dtype=torch.float64, device=device)

    def product(self, a, b, c, alpha=1.0, beta=0.0):
        p = self.F._p
        self.check(self.lib.gz_sqrtm_product(p(a), p(b), p(c), self.d, float(alpha), float(beta), self.F._stream()),
                   "sqrtm_product")

    def product_pair(self, a0, b0, c0, a1, b1, c1):
        p = self.F._p
        self.check(self.lib.gz_sqrtm_product_pair(p(a0), p(b0), p(c0), 1.0, 0.0, p(a1), p(b1), p(c1), 1.0, 0.0, self.d,
                                                  self.F._stream()), "sqrtm_product_pair")

    def trace_norm(self, a):
        """(trace(a), |a|_F^2) on the host: two launches and the 16-byte read-back."""
        p = self.F._p
        self.check(self.lib.gz_sqrtm_trace_norm(p(a), self.d, p(self.stats), p(self.ws), self.ws_bytes,
                                                self.F._stream()), "sqrtm_trace_norm")
        tr, f2 = self.stats.tolist()
        return tr, f2


def _newton_schulz_device(a, launch, maxit=NS_MAXIT):
    """``_newton_schulz`` on the device: the loop runs here over the launchers, three products (two of them in one
    launch) and one 16-byte read-back per iteration; five d x d work buffers allocated once.
    -> (Y: one of the work buffers, c, trace(Y), iterations, converged)."""
    d = a.shape[0]
    _, f2 = launch.trace_norm(a)
    c = float(np.sqrt(f2))
    if c == 0.0:
        return torch.zeros_like(a), 0.0, 0.0, 0, True
    if not np.isfinite(c):
        return a, c, float("nan"), 0, False
    y, z, tk, yn, zn = torch.empty((5, d, d), dtype=torch.float64, device=a.device).unbind(0)
    torch.div(a, c, out=y)
    z.zero_()
    z.diagonal().fill_(1.0)
    t, dprev = launch.trace_norm(y)[0], float("inf")
    for k in range(1, int(maxit) + 1):
        launch.product(z, y, tk, -0.5, 1.5)
        launch.product_pair(y, tk, yn, tk, z, zn)
        tn = launch.trace_norm(yn)[0]
        verdict, dk = _ns_verdict(t, tn, dprev)
        if verdict == "fail":
            return y, c, t, k, False
        if verdict == "new":
            return yn, c, tn, k, True
        if verdict == "old":
            return y, c, t, k, True
        y, yn, z, zn, t, dprev = yn, y, zn, z, tn, dk
    return y, c, t, int(maxit), False


def sqrtm_psd_device(a, maxit=NS_MAXIT):
    """The square root of a symmetric positive semi-definite fp64 device matrix by the coupled Newton-Schulz iteration
    on gz_sqrtm_product (csrc/gz_sqrtm.hip) -> (root: a device tensor of its own, iterations, converged).  No CPU
    fallback."""
    a = _square_fp64_device(a, "a")
    with torch.cuda.device(a.device):
        y, c, _, k, ok = _newton_schulz_device(a, _SqrtmLaunchers(a.shape[0], a.device), maxit)
        return y * float(np.sqrt(c)), k, ok


def frechet_distance_device(mu1, sigma1, mu2, sigma2, root1=None, maxit=NS_MAXIT):
    """``frechet_distance_newton_schulz`` on fp64 device statistics (``feature_moments_device`` makes them).  ``root1``:
    the square root of ``sigma1`` from an earlier ``sqrtm_psd_device`` call (the real set's does not change between
    epochs); its iteration count is then reported as 0.  -> (distance, (iterations, iterations), converged).  No CPU
    fallback."""
    sigma1, sigma2 = _square_fp64_device(sigma1, "sigma1"), _square_fp64_device(sigma2, "sigma2")
    d = sigma1.shape[0]
    for m in (mu1, mu2):
        if not isinstance(m, torch.Tensor) or m.dtype != torch.float64 or tuple(m.shape) != (d,):
            raise ValueError("the means must be float64 [%d] tensors" % d)
    if sigma2.shape != sigma1.shape:
        raise ValueError("the two statistics have different dimensions")
    with torch.cuda.device(sigma1.device):
        launch = _SqrtmLaunchers(d, sigma1.device)
        k1, ok1 = 0, True
        if root1 is None:
            root1, k1, ok1 = sqrtm_psd_device(sigma1, maxit)
        root1 = _square_fp64_device(root1, "root1")
        half, inner = torch.empty((2, d, d), dtype=torch.float64, device=sigma1.device).unbind(0)
        launch.product(root1, sigma2, half)
        launch.product(half, root1, inner)
        _, c, t, k2, ok2 = _newton_schulz_device(inner, launch, maxit)
        delta = (mu1 - mu2.to(mu1.device)).cpu().numpy()
        tr1, tr2 = launch.trace_norm(sigma1)[0], launch.trace_norm(sigma2)[0]
        fid = float(delta.dot(delta) + tr1 + tr2 - 2 * (np.sqrt(c) * t))
    return fid, (k1, k2), bool(ok1 and ok2)


class RealStatistics:
    """What ``evaluate_device`` reads of the real set, made ONCE per run (the set does not change between epochs): its
    fp64 codes resident on the device (KID draws its subsets from them) and their mean and covariance on the host
    (``frechet_distance``'s operands).  ``mu`` / ``sigma``: statistics already known (an ``inception_cache.npz``);
    without them one gz_feature_moments call.  ``device_root`` (``fid_on_device``): the statistics as device tensors and
    the square root of ``sigma``, made on first use and kept."""

    def __init__(self, real_act, device, mu=None, sigma=None):
        self.codes = device_codes(real_act, device)
        if mu is None or sigma is None:
            mean, cov = feature_moments_device(self.codes)
            mu, sigma = mean.cpu().numpy(), cov.cpu().numpy()
        self.mu, self.sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
        self._root = None
        self._radii = {}

    def radii(self, k):
        """The real codes' k-nearest-neighbour radii (``knn_radii_device``) as an fp64 device tensor, made once per run
        and ``k`` and kept."""
        k = int(k)
        if k not in self._radii:
            self._radii[k] = knn_radii_device(self.codes, k)
        return self._radii[k]

    def device_root(self):
        """-> (mu, sigma, root of sigma: fp64 device tensors, iterations, converged); one ``sqrtm_psd_device`` call per
        run."""
        if self._root is None:
            dev = self.codes.device
            mu = torch.from_numpy(np.ascontiguousarray(self.mu)).to(dev)
            sigma = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(self.sigma))).to(dev)
            self._root = (mu, sigma) + tuple(sqrtm_psd_device(sigma))
        return self._root


def device_activations(module, dump, net, batch=250):
    """The generated set's features as fp64 rows of ONE resident [n, d] device tensor (fp32 -> fp64 is exact).  ``net``:
    Inception inputs [b, 3, 299, 299] on the device -> features [b, d] on the device (``InceptionFeatures.device``)."""
    act, row = None, 0
    for x in dump.device_batches(module, batch):
        f = net(x)
        if act is None:
            act = torch.empty((dump.n_samples, f.shape[1]), dtype=torch.float64, device=f.device)
        act[row:row + f.shape[0]].copy_(f)
        row += f.shape[0]
    assert row == dump.n_samples
    return act


_fid_fallback_warned = False


def _fid_on_device(real, mean, cov):
    """The device Frechet distance with the real set's cached root; an iteration that does not converge sends THIS
    evaluation to the host's ``frechet_distance`` on the same moments (warned about once per run)."""
    global _fid_fallback_warned
    mu1, sigma1, root1, _, ok = real.device_root()
    if ok:
        fid, _, ok = frechet_distance_device(mu1, sigma1, mean, cov, root1=root1)
    if not ok:
        if not _fid_fallback_warned:
            _fid_fallback_warned = True
            import warnings
            warnings.warn("lightning_gan_zoo_amd.eval: the Newton-Schulz square root did not converge within %d iterations; "
                          "the Frechet distance of this evaluation comes from the host (scipy.linalg.sqrtm)" % NS_MAXIT)
        fid = frechet_distance(real.mu, real.sigma, mean.cpu().numpy(), cov.cpu().numpy())
    return fid


def evaluate_device(module, dump, net, real, batch=250, n_subsets=100, fid_on_device=False, classifier=None,
                    inception_splits=10, prdc_k=None):
    """``evaluate`` with everything between the generator and the metrics on the device: features at batch ``batch``
    into one resident fp64 tensor, mean / covariance through gz_feature_moments (only those two are copied to the host,
    for ``frechet_distance``), KID through ``polynomial_mmd_averages_device`` on the resident tensors -- the same subset
    draws from numpy's global generator.  ``real``: a ``RealStatistics``.  ``fid_on_device``: the moments stay on the
    device and ``frechet_distance_device`` runs with the real set's cached root.  Returns the same dict as ``evaluate``.
    ``classifier``: ``(weight, bias)`` of the classifier head in the FID weight file; the dict then gains ``"is"`` and
    ``"is_std"``, the Inception Score over ``inception_splits`` splits of the same resident generated codes
    (``inception_score_device`` -- the reference's statistic on that head, not on torchvision's ImageNet network).
    ``prdc_k``: a neighbour count; the dict then gains ``"precision"``, ``"recall"``, ``"density"`` and ``"coverage"``
    (``prdc_device`` on the same resident generated codes, the real set's radii from ``real.radii``), computed after KID
    and drawing nothing, so KID's subsets are the ones it draws without it."""
    fake = device_activations(module, dump, net, batch)
    mean, cov = feature_moments_device(fake)
    if fid_on_device:
        fid = _fid_on_device(real, mean, cov)
    else:
        fid = frechet_distance(real.mu, real.sigma, mean.cpu().numpy(), cov.cpu().numpy())
    kid = polynomial_mmd_averages_device(real.codes, fake, n_subsets=n_subsets, device=fake.device)
    out = {"fid": fid, "kid": float(kid[0].mean()), "kid_std": float(kid[0].std())}
    if classifier is not None:
        weight, bias = classifier
        out["is"], out["is_std"], _ = inception_score_device(fake, weight, bias, splits=inception_splits)
    if prdc_k is not None:
        m = prdc_device(fake, real.codes, k=prdc_k, rad_r=real.radii(prdc_k))
        out.update((key, m[key]) for key in ("precision", "recall", "density", "coverage"))
    return out


def evaluate(module, dump, feature_fn, real_act, n_subsets=100, kid_on_device=False, real_codes_device=None):
    """FID / KID of ``module.generator`` against real activations ``real_act`` (:205-238) with a pluggable
    feature extractor in place of InceptionV3's 2048-d pool features.  ``kid_on_device``: KID through
    ``polynomial_mmd_averages_device`` on the module's GPU; FID stays on the host either way.  ``real_codes_device``:
    ``device_codes(real_act, module.device)`` made once by a caller that evaluates every epoch (``real_act`` does not
    change between epochs), so that the real codes are uploaded once per run; without it they are uploaded per call."""
    fake_act = np.concatenate([np.asarray(feature_fn(img)) for img in dump.images(module)], axis=0)
    real_mu, real_sigma = activation_statistics(real_act)
    fake_mu, fake_sigma = activation_statistics(fake_act)
    fid = frechet_distance(real_mu, real_sigma, fake_mu, fake_sigma)
    if kid_on_device:
        real_codes = real_act if real_codes_device is None else real_codes_device
        kid = polynomial_mmd_averages_device(real_codes, fake_act, n_subsets=n_subsets, device=module.device)
    else:
        kid = polynomial_mmd_averages(np.asarray(real_act), fake_act, n_subsets=n_subsets)
    return {"fid": fid, "kid": float(kid[0].mean()), "kid_std": float(kid[0].std())}


def fid_from_weight_file(module, real_images_u8, weights=None, n_samples=5000, batch_size=16, n_subsets=100):
    """FID / KID end to end (reference core/callback_inception_metrics.py:183-246): the fixed latent set, the eval-mode
    generator sweep, InceptionV3 pool features on the HIP kernels with the reference's weight FILE, Frechet distance and
    KID.  ``weights``: path of pytorch-fid's ``pt_inception-2015-12-05-6726825d.pth`` (default: the ``GZ_FID_WEIGHTS``
    environment variable; the reference downloads it, metrics/inception.py:13 -- there is no network here); the file's
    sha256 prefix is verified.  ``real_images_u8``: uint8 [n, H, W, 3] real images, or None to compare the generated
    set with itself (a self-check: FID 0)."""
    import os
    from .inception import InceptionFeatures, load_fid_weights
    weights = weights or os.environ.get("GZ_FID_WEIGHTS")
    if not weights:
        raise RuntimeError("lightning_gan_zoo_amd.eval: FID needs the published Inception weight file; pass weights=<path> "
                           "or set GZ_FID_WEIGHTS (pt_inception-2015-12-05-6726825d.pth)")
    features = InceptionFeatures(load_fid_weights(weights, module.device), batch_size)
    dump = SampleDump(module, n_samples, batch_size)
    if real_images_u8 is None:
        real_act = np.concatenate([np.asarray(features(img)) for img in dump.images(module)], axis=0)
    else:
        real_act = features(real_images_u8)
    return evaluate(module, dump, features, real_act, n_subsets=n_subsets)


# ---------------------------------------------------------------------------------------------------------
# sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018, section 5 and appendix).
# The reference has no such metric: the functions below ARE its definition here.  Numpy fp64 yardsticks first, then the
# same statistic on csrc/gz_swd.hip.
# ---------------------------------------------------------------------------------------------------------
SWD_SIZES = (16, 32, 64, 128)
SWD_TAPS = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
SWD_PATCH = 7


def swd_level_sizes(size):
    """S, S/2, .., 16."""
    if size not in SWD_SIZES:
        raise ValueError("the sliced Wasserstein distance takes square images of size %s, got %r" % (SWD_SIZES, size))
    return [size >> l for l in range(SWD_SIZES.index(size) + 1)]


def _swd_mirror(idx, n):
    idx = np.abs(idx)
    return np.where(idx >= n, 2 * n - 2 - idx, idx)


def _swd_filter(x, axis, taps):
    """The 5 taps along ``axis`` with mirror border (scipy 'mirror', torch 'reflect'), t = 0 .. 4 in order."""
    n = x.shape[axis]
    out = np.zeros_like(x)
    for t in range(5):
        out = out + taps[t] * np.take(x, _swd_mirror(np.arange(n) + t - 2, n), axis=axis)
    return out


def swd_down(x):
    x = np.asarray(x, dtype=np.float64)
    return _swd_filter(_swd_filter(x, -1, SWD_TAPS)[..., ::2], -2, SWD_TAPS)[..., ::2, :]


def swd_up(y):
    y = np.asarray(y, dtype=np.float64)
    rows = np.zeros(y.shape[:-2] + (2 * y.shape[-2], y.shape[-1]))
    rows[..., ::2, :] = y
    rows = _swd_filter(rows, -2, 2.0 * SWD_TAPS)
    full = np.zeros(rows.shape[:-1] + (2 * y.shape[-1],))
    full[..., ::2] = rows
    return _swd_filter(full, -1, 2.0 * SWD_TAPS)


def laplacian_pyramid(images):
    """[N, C, S, S] -> the fp64 Laplacian levels of size S, S/2, .., 16: L_l = G_l - up(G_l+1), the last one G itself."""
    g = np.asarray(images, dtype=np.float64)
    if g.ndim != 4 or g.shape[2] != g.shape[3]:
        raise ValueError("images must be [N, C, S, S], got %s" % (g.shape,))
    levels = []
    for _ in swd_level_sizes(g.shape[2])[:-1]:
        nxt = swd_down(g)
        levels.append(g - swd_up(nxt))
        g = nxt
    return levels + [g]


def _swd_check_positions(pos, n, h):
    pos = np.asarray(pos)
    if pos.ndim != 3 or pos.shape[0] != n or pos.shape[2] != 2 or pos.shape[1] < 1:
        raise ValueError("positions must be [n = %d, P >= 1, 2] patch centres, got %s" % (n, pos.shape))
    if pos.min() < 3 or pos.max() >= h - 3:
        raise ValueError("patch centres must lie in [3, %d)" % (h - 3))
    return pos.astype(np.int64)


def swd_descriptors(level, positions):
    """[n, C, H, H] and centres [n, P, 2] (cy, cx) -> [n * P, 49 C]: row image * P + patch, element (channel, dy, dx)."""
    level = np.asarray(level, dtype=np.float64)
    n, c, h, _ = level.shape
    pos = _swd_check_positions(positions, n, h)
    off = np.arange(-3, 4)
    ys = pos[:, :, 0, None, None, None] + off[None, None, None, :, None]
    xs = pos[:, :, 1, None, None, None] + off[None, None, None, None, :]
    d = level[np.arange(n)[:, None, None, None, None], np.arange(c)[None, None, :, None, None], ys, xs]
    return d.reshape(n * pos.shape[1], c * SWD_PATCH * SWD_PATCH)


def swd_channel_statistics(desc, channels):
    """Mean and population standard deviation per channel over all values of a descriptor set, taken of v - v0 with v0
    the channel's first value (the device does the same): a constant channel then has a deviation of exactly 0, whatever
    its value -- summing n copies of it and dividing by n need not give it back."""
    d = np.asarray(desc, dtype=np.float64).reshape(len(desc), channels, -1)
    v0 = d[0, :, 0]
    shifted = d - v0[None, :, None]
    return v0 + shifted.mean(axis=(0, 2)), shifted.std(axis=(0, 2))


def swd_normalise(desc, channels):
    """(d - mean_c) / std_c per channel; a standard deviation of exactly 0 divides by 1 (a collapsed generator gets a
    finite number, not NaN)."""
    mean, std = swd_channel_statistics(desc, channels)
    d = np.asarray(desc, dtype=np.float64).reshape(len(desc), channels, -1)
    return ((d - mean[None, :, None]) / np.where(std == 0.0, 1.0, std)[None, :, None]).reshape(len(desc), -1)


def sliced_wasserstein(desc_a, desc_b, directions, repeats=1):
    """Two descriptor sets [rows, D] and unit directions [repeats * dirs, D]: every direction's projections of either set
    sorted ascending; per repeat the mean over rows and directions of |a - b|; the mean over repeats."""
    a, b = np.asarray(desc_a, dtype=np.float64), np.asarray(desc_b, dtype=np.float64)
    dirs = np.asarray(directions, dtype=np.float64)
    if a.shape != b.shape:
        raise ValueError("the two sets must have equal shapes, got %s and %s" % (a.shape, b.shape))
    if dirs.ndim != 2 or dirs.shape[1] != a.shape[1] or dirs.shape[0] % int(repeats):
        raise ValueError("directions must be [repeats * dirs, %d], got %s" % (a.shape[1], dirs.shape))
    pa, pb = np.sort(a.dot(dirs.T), axis=0), np.sort(b.dot(dirs.T), axis=0)
    per = np.abs(pa - pb).reshape(a.shape[0], int(repeats), -1).mean(axis=(0, 2))
    return float(per.mean())


def _swd_result(sizes, values):
    out = {"swd_%d" % s: float(v) for s, v in zip(sizes, values)}
    out["swd"] = float(np.mean(values))
    return out


def swd(images_a, images_b, positions, directions, repeats=1):
    """The whole statistic in numpy fp64.  ``positions[l]`` [n, P, 2] and ``directions[l]`` [repeats * dirs, 49 C] per
    level (``SwdPlan`` draws them) -> {"swd_<size>": 1000 * distance per level, "swd": their mean}."""
    la, lb = laplacian_pyramid(images_a), laplacian_pyramid(images_b)
    channels, values = la[0].shape[1], []
    for a, b, pos, dirs in zip(la, lb, positions, directions):
        da, db = swd_normalise(swd_descriptors(a, pos), channels), swd_normalise(swd_descriptors(b, pos), channels)
        values.append(1000.0 * sliced_wasserstein(da, db, dirs, repeats))
    return _swd_result([a.shape[2] for a in la], values)


class SwdPlan:
    """Every draw of the metric, made once from a private ``numpy.random.Generator(PCG64(seed))``: per level the patch
    centres [n, P, 2] (integers uniform in [3, H - 3), one table for both sets) and ``repeats * dirs`` unit directions
    (standard normal, scaled to unit length in fp64, stored fp32); with ``module``, the latents of the generated set from
    ``module.noise_distn`` under ``torch.random.fork_rng`` seeded from the same generator.  numpy's and torch's global
    generators are left as they were.  The same draws every epoch keep the curve free of resampling noise."""

    def __init__(self, size, channels, n_images, patches=128, dirs=128, repeats=4, seed=0, module=None):
        self.size, self.channels, self.n = int(size), int(channels), int(n_images)
        self.patches, self.dirs, self.repeats, self.seed = int(patches), int(dirs), int(repeats), int(seed)
        self.sizes = swd_level_sizes(self.size)
        if self.channels not in (1, 3) or min(self.n, self.patches, self.dirs, self.repeats) < 1:
            raise ValueError("SwdPlan: channels must be 1 or 3 and every count at least 1")
        rng = np.random.Generator(np.random.PCG64(self.seed))
        self.positions = [rng.integers(3, h - 3, size=(self.n, self.patches, 2)).astype(np.int32) for h in self.sizes]
        self.directions = []
        for _ in self.sizes:
            d = rng.standard_normal((self.repeats * self.dirs, SWD_PATCH * SWD_PATCH * self.channels))
            self.directions.append((d / np.sqrt((d * d).sum(axis=1, keepdims=True))).astype(np.float32))
        self.latents = None
        if module is not None:
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(int(rng.integers(0, 2 ** 62)))
                self.latents = module.noise_distn.sample((self.n, module.cfg.model.noise_dim))
        self._device = {}

    def on(self, device):
        """(positions as int32 [n * P, 2], directions as fp32) per level on ``device``, uploaded once."""
        key = str(device)
        if key not in self._device:
            self._device[key] = ([torch.from_numpy(p.reshape(-1, 2)).to(device) for p in self.positions],
                                 [torch.from_numpy(d).to(device) for d in self.directions])
        return self._device[key]


def _swd_images(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("lightning_gan_zoo_amd.eval: the device %s runs on the HIP kernels; its input is not a GPU "
                           "tensor and there is no fallback (use eval.swd)" % what)
    if x.dim() != 4 or x.dtype != torch.float32 or x.shape[2] != x.shape[3] or x.shape[1] not in (1, 3):
        raise ValueError("images must be float32 [N, C in (1, 3), S, S], got %s %s" % (x.dtype, tuple(x.shape)))
    swd_level_sizes(x.shape[2])
    return x if x.is_contiguous() else x.contiguous()


def laplacian_pyramid_device(images):
    """``laplacian_pyramid`` of fp32 device images [N, C, S, S]: one gz_swd_pyramid launch, the levels as views of one
    packed fp32 buffer.  No CPU fallback."""
    import ctypes
    from . import functional as F
    from ._lib import check, lib
    x = _swd_images(images, "Laplacian pyramid")
    n, c, s, _ = x.shape
    count, offsets = ctypes.c_int(0), (ctypes.c_longlong * 5)()
    check(lib.gz_swd_pyramid_describe(n, c, s, ctypes.byref(count), offsets), "swd_pyramid_describe")
    with torch.cuda.device(x.device):
        out = torch.empty((offsets[count.value],), dtype=torch.float32, device=x.device)
        check(lib.gz_swd_pyramid(F._p(x), n, c, s, F._p(out), out.numel(), F._stream()), "swd_pyramid")
    return [out[offsets[l]:offsets[l + 1]].view(n, c, s >> l, s >> l) for l in range(count.value)]


def swd_sort_plan(rows):
    """-> (block length, padded length, block passes, global passes) of gz_swd_sort_columns for ``rows`` keys a column."""
    import ctypes
    from ._lib import check, lib
    block, padded, bp, gp = ctypes.c_int(0), ctypes.c_longlong(0), ctypes.c_int(0), ctypes.c_int(0)
    check(lib.gz_swd_sort_plan(int(rows), ctypes.byref(block), ctypes.byref(padded), ctypes.byref(bp), ctypes.byref(gp)),
          "swd_sort_plan")
    return block.value, padded.value, bp.value, gp.value


def swd_sorted_projections_device(level, pos, dirs):
    """One level [n, C, H, H] (fp32, device), centres [n * P, 2] (int32, device) and directions [ndirs, 49 C] (fp32,
    device) -> [ndirs, padded] fp32: every direction's projections of the normalised descriptors, sorted ascending, +inf
    beyond the n * P rows.  gz_swd_channel_stats, gz_swd_project, gz_swd_sort_columns; nothing reaches the host."""
    from . import functional as F
    from ._lib import check, lib
    level = _swd_images(level, "sorted projections")
    n, c, h, _ = level.shape
    for t, dtype, what in ((pos, torch.int32, "centres"), (dirs, torch.float32, "directions")):
        if (not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 2 or t.device != level.device
                or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous 2-D %s tensor on %s (SwdPlan.on makes them)" % (what, dtype, level.device))
    rows, ndirs = pos.shape[0], dirs.shape[0]
    if pos.shape[1] != 2 or rows % n or rows < 1 or ndirs < 1 or dirs.shape[1] != SWD_PATCH * SWD_PATCH * c:
        raise ValueError("centres must be [n * P, 2] and directions [ndirs, %d]" % (SWD_PATCH * SWD_PATCH * c))
    p = rows // n
    pitch = max(swd_sort_plan(rows)[1], 4)             # (the sort reads 16 bytes at a time)
    with torch.cuda.device(level.device):
        stats = torch.empty((2 * c,), dtype=torch.float64, device=level.device)
        ws_bytes = lib.gz_swd_channel_stats_workspace_bytes(n, c, h, p)
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=level.device)
        check(lib.gz_swd_channel_stats(F._p(level), n, c, h, F._p(pos), p, F._p(stats), F._p(ws), ws_bytes, F._stream()),
              "swd_channel_stats")
        proj = torch.empty((ndirs, pitch), dtype=torch.float32, device=level.device)
        check(lib.gz_swd_project(F._p(level), n, c, h, F._p(pos), p, F._p(stats), F._p(dirs), ndirs, F._p(proj), pitch,
                                 F._stream()), "swd_project")
        check(lib.gz_swd_sort_columns(F._p(proj), rows, ndirs, pitch, F._stream()), "swd_sort_columns")
    return proj


def swd_distance_device(sorted_a, sorted_b, rows, repeats=1):
    """Two results of ``swd_sorted_projections_device`` -> the mean over repeats of the mean |a - b| over rows and the
    repeat's directions: gz_swd_distance, ``repeats`` doubles copied back."""
    from . import functional as F
    from ._lib import check, lib
    if sorted_a.shape != sorted_b.shape or sorted_a.shape[0] % int(repeats):
        raise ValueError("the two sets must have equal shapes with repeats * dirs directions, got %s and %s"
                         % (tuple(sorted_a.shape), tuple(sorted_b.shape)))
    per = sorted_a.shape[0] // int(repeats)
    with torch.cuda.device(sorted_a.device):
        out = torch.empty((int(repeats),), dtype=torch.float64, device=sorted_a.device)
        ws_bytes = lib.gz_swd_distance_workspace_bytes(rows, per, int(repeats))
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=sorted_a.device)
        check(lib.gz_swd_distance(F._p(sorted_a), rows, F._p(sorted_b), rows, per, int(repeats), sorted_a.shape[1],
                                  F._p(out), F._p(ws), ws_bytes, F._stream()), "swd_distance")
        sums = out.cpu().numpy()
    return float((sums / (float(rows) * per)).mean())


def sliced_wasserstein_device(level_a, level_b, pos, dirs, repeats=1, sorted_b=None):
    """``sliced_wasserstein(swd_normalise(swd_descriptors(..)), ..)`` of two fp32 device levels with device centres and
    directions.  ``sorted_b``: the second set's sorted projections when the caller keeps them.  No CPU fallback."""
    for t in (level_a, level_b):
        _swd_images(t, "sliced Wasserstein distance")
    if level_a.shape != level_b.shape:
        raise ValueError("the two sets must have equal shapes, got %s and %s" % (tuple(level_a.shape), tuple(level_b.shape)))
    sa = swd_sorted_projections_device(level_a, pos, dirs)
    sb = swd_sorted_projections_device(level_b, pos, dirs) if sorted_b is None else sorted_b
    return swd_distance_device(sa, sb, pos.shape[0], repeats)


class RealPyramid:
    """The real set's side of the metric, made once per run: its Laplacian levels resident in fp32, and its sorted
    projections per level, made at the first evaluation and kept while all levels' fit under ``cache_gb``; above the
    budget they are recomputed from the resident levels at every evaluation (the same launches: the same bits)."""

    def __init__(self, images, plan, cache_gb=16):
        x = _swd_images(images, "sliced Wasserstein distance")
        if tuple(x.shape) != (plan.n, plan.channels, plan.size, plan.size):
            raise ValueError("the real set must be %s, got %s" % ((plan.n, plan.channels, plan.size, plan.size),
                                                                  tuple(x.shape)))
        self.plan, self.levels = plan, laplacian_pyramid_device(x)
        padded = swd_sort_plan(plan.n * plan.patches)[1]
        self.cache_bytes = len(self.levels) * plan.repeats * plan.dirs * padded * 4
        self.cached = self.cache_bytes <= float(cache_gb) * 2 ** 30
        self._sorted = {}

    def sorted(self, l):
        if l in self._sorted:
            return self._sorted[l]
        pos, dirs = self.plan.on(self.levels[l].device)
        s = swd_sorted_projections_device(self.levels[l], pos[l], dirs[l])
        if self.cached:
            self._sorted[l] = s
        return s


def swd_device(images_a, images_b, positions, directions, repeats=1):
    """``swd`` on fp32 device images: gz_swd_pyramid per set, then per level the statistics, projections, sorts and the
    distance on the device; ``repeats`` doubles per level travel to the host.  ``positions`` / ``directions`` as for
    ``swd`` (numpy; uploaded here).  No CPU fallback."""
    a, b = _swd_images(images_a, "sliced Wasserstein distance"), _swd_images(images_b, "sliced Wasserstein distance")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("the two sets must have equal shapes on one device, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    la, lb = laplacian_pyramid_device(a), laplacian_pyramid_device(b)
    values = []
    for x, y, pos, dirs in zip(la, lb, positions, directions):
        pos = torch.from_numpy(np.ascontiguousarray(_swd_check_positions(pos, x.shape[0], x.shape[2]).reshape(-1, 2)
                                                    .astype(np.int32))).to(a.device)
        dirs = torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float32)).to(a.device)
        values.append(1000.0 * sliced_wasserstein_device(x, y, pos, dirs, repeats))
    return _swd_result([x.shape[2] for x in la], values)


@torch.no_grad()
def evaluate_swd(module, plan, real, batch=250):
    """The metric of ``module.generator`` against ``real`` (a ``RealPyramid``): the eval-mode sweep over ``plan.latents``
    -- the raw tanh output, not clamped -- the pyramid and per level one distance.  The module's mode, numpy's global
    generator (a generator with ``sample_view`` draws from it: seeded from the plan's seed inside, restored afterwards)
    and torch's generators are left as they were.  -> {"swd_<size>": .., "swd": mean}."""
    from . import functional as F
    if plan.latents is None:
        raise ValueError("the plan was built without a module: it holds no latents")
    gen = module.generator
    if hasattr(gen, "drop_prefetched_view"):
        # where the LIVE generator is swept (no averaging), its view prefetched for the next training step must be rolled
        # back BEFORE numpy's state is saved: the sweep's forwards would otherwise discard it under the plan's seed without
        # rolling back, and the next step would draw another view than a run without the metric.  (The averaged copy
        # never holds one -- averaging.SCRATCH_ATTRS -- so there this does nothing and the live prefetch stays valid.)
        gen.drop_prefetched_view()
    host_state = np.random.get_state()
    was_training = module.training
    module.eval()
    try:
        np.random.seed(plan.seed % (2 ** 32))
        with torch.random.fork_rng(devices=[module.device] if torch.device(module.device).type == "cuda" else []):
            fake = torch.cat([F._req(module.generator(z.to(module.device)).detach().float(), "samples")
                              for z in torch.split(plan.latents, int(batch))])
    finally:
        module.train(was_training)
        np.random.set_state(host_state)
    fake_levels = laplacian_pyramid_device(fake)
    del fake
    pos, dirs = plan.on(fake_levels[0].device)
    values = []
    for l, level in enumerate(fake_levels):
        sorted_fake = swd_sorted_projections_device(level, pos[l], dirs[l])
        values.append(1000.0 * swd_distance_device(sorted_fake, real.sorted(l), pos[l].shape[0], plan.repeats))
    return _swd_result(plan.sizes, values)
