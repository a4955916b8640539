"""The statistic of the device T3: are two sets of batch images estimates of the same image?  (numpy only: no GPU, no
oracle, no scipy.)

`check(ref, dev, what, ref_spp, dev_spp)` takes two arrays [B, H, W, 3] of per-batch pixel means, B = 16 independent
batches each — the reference's mt19937 stream on one side, the code under test on the other — and each side's samples
per pixel and batch, and holds them to four conditions.  It returns the measured figures and raises T3Error, naming `what`,
every condition that failed, the channel and (for a pixel condition) the pixel.  A term is one (pixel, channel).

Notation.  For a term, x_1..x_B are the reference's batch means (variance s2x, estimated with B - 1 degrees of freedom),
y_1..y_B the device's (s2y), d = mean(y) - mean(x).  If both sides estimate the same expectation, d has variance
(sigma2_x + sigma2_y) / B, and

    F = d^2 / (s2x / B + s2y / B)

is the square of Welch's t: approximately F(1, nu) with the Welch-Satterthwaite degrees of freedom

    nu = (sigma2_x + sigma2_y)^2 / (sigma2_x^2 / (B - 1) + sigma2_y^2 / (B - 1)) = (B - 1) (1 + r)^2 / (1 + r^2),

r = sigma2_y / sigma2_x.  r is the ratio of the two sides' samples per batch, the same for every term, so it is measured
once, pooled: r = sum s2y / sum s2x over the non-deterministic terms.  15 <= nu <= 30 for B = 16.

1. Deterministic terms.  A term whose reference batches spread (max - min) by less than tol = FLOOR x max(|mean|, 1e-3),
   FLOOR = 1e-9, showed no Monte-Carlo noise: all the reference's samples of it have one value v (the sky's blue is
   exactly 1).  No F can be formed there.  (The floor is not zero because a sum of 256 equal values and a sum of 4096
   round differently, and the fast build contracts: both are some 1e-16 x the value, seven decades below the floor; the
   smallest spread of a term with noise at these sizes is 5.6e-8 x its mean.)  At most DET_CAP = 15 % of the terms may be
   of this class, or the statistic would be looking at too little of the image.  On such a term:
   a. if the device's batches are spread-free too (max - min < tol), every one of them must be within tol of v;
   b. if they are not, the device saw samples that differ from v.  That happens between two correct sides: a pixel on a
      silhouette whose blue is 0.5 in all but one sample in 10^4 is spread-free in the reference's n_ref = 16 x 256
      samples and not in the device's n_dev = 16 x 4096 (12 of 849 such terms between two mt19937 streams of the static
      cover, 34 against the Philox oracle at 4096; some with an odd sample in EVERY device batch, so no count of clean
      batches can be asserted).  What the reference does bound is how often: with p the probability that a sample of
      the term differs from v, the reference is spread-free with probability (1 - p)^n_ref <= exp(-p n_ref), so
      "some term with p > p* is spread-free" has probability <= ALPHA / 2 over all N_terms for p* = L / n_ref,
      L = ln(2 N_terms / ALPHA).  With p <= p* the number K of odd samples among the device's n_dev is at most
      Binomial(n_dev, p*), mean lam = L n_dev / n_ref, and by Chernoff's bound P(K >= (1 + e) lam) <= exp(-lam e^2 /
      (2 + e)) = ALPHA / (2 N_terms) for e = (rho + sqrt(rho^2 + 8 rho)) / 2, rho = n_ref / n_dev.  A sample lies in
      [0, sample_range] (no emitters, the sky and every attenuation <= 1), so an odd sample moves the device mean by at
      most sample_range / n_dev:   |mean(y) - v| <= (1 + e) (L / n_ref) sample_range   (5.6e-3 for 4096 against 65536
      samples, 1.2e-2 for 4096 against 4096).  Coarse — it is all that 4096 equal samples can say about the 4097th — and
      of the size of what condition 4 resolves on a single noisy term.  The count of these terms is returned.
2. Image means, per channel.  m_b = the mean over the whole image of batch b, 16 numbers per side; SE^2 = var(m_x) / B +
   var(m_y) / B.  |mean(m_y) - mean(m_x)| <= q_t SE, q_t the two-sided 0.1 % / 3 quantile (three channels) of Student's
   t at the Welch degrees of freedom of these two samples; and <= ABS_MEANS = 0.05 / 255 whatever the SE.
   q_t SE is the smallest bias of the image mean the check refuses; it is returned (`resolution`).
3. The mean of F over the non-deterministic terms.  E F(1, nu) = nu / (nu - 2), Var F(1, nu) = 2 nu^2 (nu - 1) /
   ((nu - 2)^2 (nu - 4)).  Terms of different pixels come from disjoint samples and are independent; the three channels
   of a pixel come from the same paths and are not.  Taking them as fully dependent bounds the variance of the mean from
   above: Var / N_pixels, N_pixels the pixels with a non-deterministic term.  So
       | mean F - nu / (nu - 2) | <= Z sqrt(Var / N_pixels),   Z = 3.2905, the two-sided 0.1 % normal quantile
   (2,400 pixels: the mean is normal to the accuracy that matters).  The upper side refuses errors spread over many
   pixels, each too small for condition 4; the LOWER side refuses a device image that is closer to the reference than
   independent samples can be — the reference itself, a copy, an average that contains it.
4. The largest F.  <= the F(1, nu) quantile at 0.001 / N_terms (Bonferroni), N_terms = 3 H W: every term of the image,
   a few more than are tested, which moves the quantile up by less than 1 %.

How far F(1, nu) holds.  It presumes normal batch means.  A batch mean of 256 samples of a path tracer is skewed (rare
bright paths), and for a sample of B values of skewness g the mean of t^2 is above nu / (nu - 2) by about 3 g^2 / B:
with the device at 4096 spp F is nearly the reference's own one-sample t^2, and the measured mean F of the cover scenes
sits 0.05 - 0.07 above E (1.19 - 1.21 against 1.134; suzanne 1.14; two mt19937 sets against each other 1.05 - 1.10
against 1.071) — inside the band, whose half width is 0.12, and the same for every correct device, since the reference
is fixed.  The band is not widened for it: the upper side is that much sharper than stated, the lower side that much
blunter — the mean of the reference and the device, planted as the device, gives 0.28.

Quantiles.  F(1, nu) at 1 - p is the square of Student's t at 1 - p / 2.  The t quantiles below were computed once with
scipy 1.15 (scipy.stats.t.isf) at nu = 15 .. 30 and are interpolated linearly in nu (error < 1e-3 relative, on the
generous side: the quantile is convex in nu); tests/test_t3_stats_host.py recomputes them where scipy is installed.
T_MAXF is for N_terms = 7200 (60 x 40 x 3), the frame of tests/t3_ref.py; `check` refuses other frames.

How sharp.  With the reference at 16 x 256 and the device at 16 x 4096 samples per pixel the SE of an image mean is
2.4e-5 .. 4.1e-5 of linear radiance and q_t about 4.4: a bias of 1.1e-4 .. 1.85e-4 = 0.03 .. 0.047 / 255 of a channel's
image mean is refused (the measured figures of every case are in DESIGN.md section 3).  Every condition is at the 0.1 %
level, so a correct device fails a case with probability <= 0.5 % — and then fails it every time, since both sides are
deterministic: a failure is to be understood, never rerun away.
"""
from __future__ import annotations

import math

import numpy as np

B = 16
FLOOR = 1e-9
FLOOR_SCALE = 1e-3
DET_CAP = 0.15
ABS_MEANS = 0.05 / 255
ALPHA = 0.001
Z = 3.2905267314918945  # scipy.stats.norm.isf(0.001 / 2)
NU = tuple(range(15, 31))
# scipy.stats.t.isf(0.001 / 3 / 2, nu): the two-sided 0.1 % / 3 quantile
T_MEANS = (4.620249, 4.541989, 4.474672, 4.416165, 4.364854, 4.319495, 4.279114, 4.242937, 4.210343, 4.180826, 4.153972,
           4.129437, 4.106933, 4.086221, 4.067093, 4.049376)
# scipy.stats.t.isf(0.001 / 7200 / 2, nu): its square is scipy.stats.f.isf(0.001 / 7200, 1, nu)
T_MAXF_TERMS = 7200
T_MAXF = (9.245214, 8.883448, 8.580278, 8.322791, 8.101561, 7.909553, 7.741422, 7.593036, 7.461155, 7.343203, 7.237109,
          7.14119, 7.054064, 6.974586, 6.901801, 6.834904)
CHANNELS = "RGB"


class T3Error(AssertionError):
    """.conditions: the names of the conditions that failed ("deterministic", "deterministic (odd samples)",
    "deterministic share", "image mean", "image mean (absolute)", "mean F low", "mean F high", "max F"); .figures: what
    check() would have returned."""

    def __init__(self, msg, conditions, figures):
        super().__init__(msg)
        self.conditions, self.figures = conditions, figures


def t_quantile(table, nu):
    if not NU[0] - 1e-9 <= nu <= NU[-1] + 1e-9:
        raise ValueError(f"no quantile for {nu} degrees of freedom")
    return float(np.interp(nu, NU, table))  # (clamps the rounding of nu = 15 or 30)


def welch_nu(vx, vy, n=B):
    """Welch-Satterthwaite degrees of freedom of two samples of n with variances vx, vy (both means' variances / n)."""
    return (n - 1) * (vx + vy) ** 2 / (vx * vx + vy * vy)


def f_moments(nu):
    """(E, Var) of F(1, nu)."""
    return nu / (nu - 2.0), 2.0 * nu * nu * (nu - 1.0) / ((nu - 2.0) ** 2 * (nu - 4.0))


def odd_sample_bound(n_ref, n_dev, n_terms, sample_range=1.0):
    """Condition 1b: the most the device mean of a term may differ from the one value of all n_ref reference samples."""
    L = math.log(2.0 * n_terms / ALPHA)
    rho = n_ref / n_dev
    e = (rho + math.sqrt(rho * rho + 8.0 * rho)) / 2.0
    return (1.0 + e) * (L / n_ref) * sample_range


def check(ref_batches, dev_batches, what, ref_spp, dev_spp, sample_range=1.0):
    ref, dev = np.asarray(ref_batches, dtype=np.float64), np.asarray(dev_batches, dtype=np.float64)
    if ref.shape != dev.shape or ref.ndim != 4 or ref.shape[0] != B or ref.shape[3] != 3:
        raise ValueError(f"{what}: batches {ref.shape} against {dev.shape}; want two of [{B}, H, W, 3]")
    if ref[0].size != T_MAXF_TERMS:
        raise ValueError(f"{what}: {ref[0].size} terms; T_MAXF is the quantile for {T_MAXF_TERMS}")
    if not (np.isfinite(ref).all() and np.isfinite(dev).all()):
        raise T3Error(f"{what}: a batch mean is not finite", ["finite"], {})
    failed, lines = [], []

    def fail(cond, text):
        failed.append(cond)
        lines.append(f"{cond}: {text}")

    def where(flat):
        i, j, c = np.unravel_index(int(flat), ref.shape[1:])
        return f"pixel (row {i}, column {j}) channel {CHANNELS[c]}"

    mx, my = ref.mean(axis=0), dev.mean(axis=0)
    # 1. deterministic terms
    tol = FLOOR * np.maximum(np.abs(mx), FLOOR_SCALE)
    det = (ref.max(axis=0) - ref.min(axis=0)) < tol
    share = float(det.mean())
    if share > DET_CAP:
        fail("deterministic share", f"{share:.4f} of the terms have no spread in the reference (cap {DET_CAP})")
    quiet = det & ((dev.max(axis=0) - dev.min(axis=0)) < tol)  # 1a: spread-free on both sides
    off = np.where(quiet, np.abs(dev - mx).max(axis=0) / tol, 0.0)
    if (off > 1.0).any():
        k = off.argmax()
        fail("deterministic", f"{int((off > 1.0).sum())} terms without spread on either side differ; worst {where(k)}: "
             f"device {dev.reshape(B, -1)[:, k].min()!r} .. {dev.reshape(B, -1)[:, k].max()!r} against {mx.flat[k]!r}")
    odd = det & ~quiet  # 1b: samples the reference did not see
    odd_bound = odd_sample_bound(B * ref_spp, B * dev_spp, ref[0].size, sample_range)
    odd_off = np.where(odd, np.abs(my - mx), 0.0)
    if (odd_off > odd_bound).any():
        k = odd_off.argmax()
        fail("deterministic (odd samples)", f"{int((odd_off > odd_bound).sum())} terms without spread in the reference differ "
             f"by more than {odd_bound:.3e} in the device mean; worst {where(k)}: {my.flat[k]!r} against {mx.flat[k]!r}")
    # 2. image means
    ix, iy = ref.mean(axis=(1, 2)), dev.mean(axis=(1, 2))  # [B, 3]
    vx, vy = ix.var(axis=0, ddof=1) / B, iy.var(axis=0, ddof=1) / B
    diff = iy.mean(axis=0) - ix.mean(axis=0)
    se = np.sqrt(vx + vy)
    qt = np.array([t_quantile(T_MEANS, welch_nu(vx[c], vy[c])) if vx[c] + vy[c] > 0 else T_MEANS[0] for c in range(3)])
    for c in range(3):
        if abs(diff[c]) > qt[c] * se[c]:
            fail("image mean", f"channel {CHANNELS[c]}: device - reference = {diff[c]:.3e} = {diff[c] / se[c]:.2f} SE "
                 f"(SE {se[c]:.3e}, allowed {qt[c]:.2f} SE)")
        if abs(diff[c]) > ABS_MEANS:
            fail("image mean (absolute)", f"channel {CHANNELS[c]}: device - reference = {diff[c]:.3e} "
                 f"(allowed 0.05 / 255 = {ABS_MEANS:.3e})")
    # 3, 4. F over the non-deterministic terms
    live = ~det
    s2x, s2y = ref.var(axis=0, ddof=1)[live], dev.var(axis=0, ddof=1)[live]
    r = float(s2y.sum() / s2x.sum())
    nu = (B - 1) * (1.0 + r) ** 2 / (1.0 + r * r)
    F = (my[live] - mx[live]) ** 2 / (s2x / B + s2y / B)
    n_pixels = int(live.any(axis=-1).sum())
    e, var = f_moments(nu)
    half = Z * math.sqrt(var / n_pixels)
    mean_f, max_f = float(F.mean()), float(F.max())
    by_channel = [float(F[np.nonzero(live)[2] == c].mean()) for c in range(3)]
    if mean_f < e - half:
        fail("mean F low", f"{mean_f:.4f}, below {e:.4f} - {half:.4f} (nu {nu:.2f}, {n_pixels} pixels; channels "
             f"{by_channel}): the device image is closer to the reference than independent samples can be")
    if mean_f > e + half:
        fail("mean F high", f"{mean_f:.4f}, above {e:.4f} + {half:.4f} (nu {nu:.2f}, {n_pixels} pixels; channels "
             f"{by_channel})")
    bound = t_quantile(T_MAXF, nu) ** 2
    if max_f > bound:
        k = np.flatnonzero(live)[F.argmax()]
        fail("max F", f"{max_f:.1f} at {where(k)}, above {bound:.1f} (nu {nu:.2f}); {int((F > bound).sum())} terms above; "
             f"device {my.flat[k]:.6f} against {mx.flat[k]:.6f}")
    figures = dict(det_share=share, odd_terms=int(odd.sum()), odd_max=float(odd_off.max()), odd_bound=odd_bound,
                   q_t_se=(qt * se).tolist(), diff=diff.tolist(), se=se.tolist(), ratio=(np.abs(diff) / se).tolist(), q_t=qt.tolist(),
                   resolution=float(np.minimum(qt * se, ABS_MEANS).max()), r=r, nu=nu, mean_f=mean_f,
                   mean_f_band=(e - half, e + half), mean_f_channels=by_channel, max_f=max_f, max_f_bound=bound,
                   n_terms=int(live.sum()), n_pixels=n_pixels)
    if failed:
        raise T3Error(f"{what}: " + "; ".join(lines), failed, figures)
    return figures


def describe(what, fig):
    """One line of the measured figures, for the tests' output."""
    return (f"{what}: SE {[f'{v:.2e}' for v in fig['se']]}, |diff| / SE {[f'{v:.2f}' for v in fig['ratio']]} "
            f"(allowed {min(fig['q_t']):.2f}), refuses a bias of {fig['resolution']:.2e} = {fig['resolution'] * 255:.3f} / 255; "
            f"r {fig['r']:.4f}, nu {fig['nu']:.2f}; mean F {fig['mean_f']:.4f} in [{fig['mean_f_band'][0]:.4f}, "
            f"{fig['mean_f_band'][1]:.4f}]; max F {fig['max_f']:.1f} <= {fig['max_f_bound']:.1f}; deterministic "
            f"{fig['det_share']:.4f}, {fig['odd_terms']} of them with odd samples (off by {fig['odd_max']:.2e} <= "
            f"{fig['odd_bound']:.2e})")
