"""-m gpu: BatchNorm1d + LeakyReLU (csrc/losses.hip), the fused discriminator tail and head (csrc/disc_tail.hip) and the column-statistics
epilogue of the weight-stationary convs (csrc/conv_ws.hip), route by route, against float64 references (tests/numerics.py: bn_stats,
bn_lrelu_fwd, bn_lrelu_bwd, tail_logits, tail_bwd, head_bwd, col_stats).

Each BatchNorm case names the kernels that must serve it, forces them with the library's switches (env_switches) and confirms them from
eegldm_debug_bn_last_route (statistics family, apply family, blocks, rows per block, TX, TY, deterministic flag); a case served by another
kernel fails.  The fused tail / head run through eegldm_debug_disc_*, which call the kernels behind the executor's eligibility check; their
template instantiation (G lanes per row, NJ chunks per lane) follows from the channel count and the storage type and is printed.  Every
check prints one `[numerics]` line, every launch one `[route]` line.  tests/test_batchnorm_numerics_cpu.py holds an fp32 model of the same
arithmetic to the same checks and plants defects that they must reject.

u = 2^-24, gamma(n) = (n + 4) u (numerics.gamma: n fp32 additions in any order, four spare roundings).  All bounds are evaluated from the
float64 reference; none is fitted.

Statistics (mean, rstd = (var + eps)^-1/2, biased var = S2 / n - mean^2: one pass about ZERO)
  The bound is that of the arithmetic these tests met: per thread, fp32 sums of x and x^2 over at most n_p elements; fp64 across the threads
  of a block; on the 4-wide route the fp64 block sum rounded to fp32 (one rounding per block partial); fp64 fold; mean and rstd cast to fp32.
    4-wide route   n_p = ceil(rows_per_block / TY)          (thread (tx, ty) owns 4 channels and the rows ty, ty + TY, ...)
    scalar route   n_p = ceil(rows_per_block / 4) + 3       (4 row lanes, whose fp32 sums are added in fp32: 3 more additions)
    e_mean = (gamma(n_p) + u) mean|x| + u |mean|
    e_var  = (gamma(n_p + 2) + u) (var + mean^2) + 2 |mean| e_mean          (x^2 rounded, then summed; mean' squared)
    e_rstd = e_var / (2 (var + eps)) + 4u                                   (relative; 4u: fp64 sqrt and division, the cast, spare)
  (the + u is the block partial's rounding and is dropped on the scalar route.)  The factor 1 + mean^2 / var is IN the bound: at a channel
  mean of 100 sigma a relative rstd error of ~1e4 x 7u = 4e-3 is allowed; each case prints the measured errors next to it.
  That arithmetic was inside this bound and still failed check B below for fp16 at 30 and 100 sigma (rstd off by 1e-5 .. 2e-4 is 0.02 .. 0.4 ulp
  of an fp16 output: up to 10 % of dx off RNE(ref) where torch's fp32 has 0.1 %; profiles/bn_numerics.txt).  The forward statistics kernels
  now sum in fp64 per thread and across the lanes of a block, and a block partial leaves as two fp32 rows (value and remainder), so their
  error is that of the two casts; the bound stays as derived, an upper bound the kernels are now far inside, and the pivot is not needed.
  From partials (the fold that follows a conv's column-statistics epilogue): against the float64 math.fsum of the very fp32 partials
  handed in, |mean' - mean| <= u |mean| and e_rstd = gamma64(nparts) (var + mean^2) / (var + eps) + 4u, gamma64(n) = (n + 4) 2^-53.
  Eval mode: the mean is the running mean, copied; rstd = rsqrtf(running_var + eps): e_rstd = 4u (the addition, rsqrtf at 1 ulp = 2u, spare).
  Running statistics: r' = (1 - m) r + m s in fp32 with m = 0.1f: 4u (0.9 |r| + 0.1 |s|) for the two constants, two products and the sum, plus
  0.1 x the error of s (s = mean: e_mean; s = unbiased var: (e_var + u var) n / (n - 1)); num_batches_tracked is exact.

Forward  y = lrelu(z), z = gamma xhat + beta (the 4-wide kernels fold it: z = fma(x, sc, sh), sc = gamma rstd, sh = beta - mean sc)
    d = |gamma| (|xhat| e_rstd + rstd e_mean) + 3u |gamma| rstd (|x| + |mean|) + 4u |z| + u |y|
  the statistics' error carried to z, the roundings of sc, sh and the fma acting on the UNcentred magnitudes, four spare, and the product
  with the slope.  LeakyReLU is continuous with slope <= 1, so d bounds y as it bounds z.  Check A: fp32 |y' - y| <= d, 16-bit outputs
  inside [RNE(y - d), RNE(y + d)].  16-bit outputs also pass check B (numerics.check_b) against torch's fp32 batch_norm + leaky_relu.
  gamma == NULL (plain LeakyReLU) is exact: x, or the fp32 product slope x rounded once to the storage type.

Mask-uncertain set  U = {|z| <= d}: the kernel's z' may have either sign there, and the backward kernels spell the mask three ways
  (ga xhat' + be <= 0 in the reduce kernels, fma(x, sc, sh) > 0 in the 4-wide apply, the head's fma chain).  A correct kernel may take
  either branch on U; U is computed from the reference and d alone and asserted to hold at most 1 % of a case's elements BEFORE the
  device result is looked at.  (bf16 at 100 sigma has ~8 distinct values per channel and a share of 2.7e-3; it is not used: bf16 runs at
  0 and 30 sigma, fp32 and f16 at 0, 30 and 100.)

Backward  dz = dy (z > 0 ? 1 : slope), S1 = sum dz, S2 = sum dz xhat, dbeta += S1, dgamma += S2, dx = sc (dz - S1 / n - xhat S2 / n)
  With |dz|~ = |dy| on {z > 0} and U, slope |dy| elsewhere, dxh = |xhat| e_rstd + rstd e_mean + 2u rstd (|x| + |mean|) the error of the
  kernel's xhat, and W(f) = sum over U of (1 - slope) |dy| f:
    bS1 = gamma(rows) sum |dz|~ + W(1)                     (slope product, partial's rounding, cast, accumulation: the four spare)
    bS2 = gamma(rows + 2) sum |dz|~ |xhat| + sum |dz|~ dxh + W(|xhat|)
    dbeta, dgamma: the same with the start value of the accumulated buffer added to the sum of magnitudes
    |dx' - dx| <= |sc| (bS1 / n + |xhat| bS2 / n + |k2| dxh) + (e_rstd + 3u) |dx| + 6u |sc| (|dz|~ + |k1| + |xhat k2|),  k = S / n
  An element of U passes with either mask value.  16-bit dx also passes check B against fp32 autograd.

Fused tail  logits = bias + sum_t sum_c w_t[c] a[l + t - 1, c], a = lrelu(bn(y)) with GIVEN statistics (the float64 ones rounded to fp32:
  e_mean = u |mean|, e_rstd = u, so the tail is judged on its own arithmetic; one case takes them from eegldm_batchnorm_lrelu_fwd)
    logits: gamma(3 C + 4) sum |w_t| (|a| + d_a) + sum |w_t| d_a,  d_a the forward bound of a
    backward: da = dl[l + 1] w_0 + dl[l] w_1 + dl[l - 1] w_2 is recomputed in fp32 (three roundings: 3u sum |dl| |w| joins |dz|~ and the
    count of every sum: gamma(rows + 3), gamma(rows + 5)); dy, dgamma, dbeta as above; dw_t = sum a dl[l - t + 1]:
    gamma(rows + 2) sum (|a| + d_a) |dl| + sum d_a |dl| (a is continuous in z: no U term); dbias = sum dl: gamma(rows) sum |dl|.
Fused head  z = b + sum_t w_t x[s l + t - 1] by an fma chain: d = gamma(3 + 4) sum |w_t x_t| + u |b|, U as above;
    dy0 = da (z > 0 ? 1 : slope); dw_t = sum dy0 x_t: gamma(rows + 2) sum |dy0|~ |x_t| + W(|x_t|); db: gamma(rows + 1) sum |dy0|~ + W(1);
    dx[i] = sum over (t, l: s l + t - 1 = i) of <dy0[l], w_t>: gamma(3 C0 + 2) of the same sum of magnitudes + W(|w_t|) scattered likewise.
Column statistics (the ST epilogue of conv_ws.hip: per-block fp32 sums of the UNROUNDED outputs y and of y^2, per column)
    reference: the float64 conv of the stored operands (+ bias), unrounded; mag_conv = the same conv of the magnitudes; the kernel's fp32
    y' is within dy = gamma(3 Cin + 4) mag_conv of y.  The returned partials are folded in float64 on the host (exact to 2^-53 nparts):
    sum:            gamma(rows + 3 Cin + 4) sum over rows of mag_conv        (the products and the row sum, one any-order fp32 sum)
    sum of squares: sum (2 |y| dy + dy^2) + gamma(rows + 2) sum y^2          (y'^2 against y^2, then rows squares summed in fp32)
  and the same partials go through eegldm_debug_bn_stats_from_parts, held to the from-parts bound above."""
import ctypes
import csv
import math
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import numerics as N

pytestmark = pytest.mark.gpu

FMT = {0: "f32", 1: "bf16", 2: "f16"}
EPS = 1e-5                              # the library's BatchNorm eps (torch's default)
SLOPE = float(np.float32(0.2))          # the value the kernels multiply by
U_CAP = 0.01
NONE, EVAL, SCALAR, VEC_FF, VEC_FOLD, PARTS = 0, 1, 2, 3, 4, 5
FAMILY = {NONE: "none (plain LeakyReLU)", EVAL: "eval", SCALAR: "scalar + fp64 atomics", VEC_FF: "4-wide partials + fold_finalize",
          VEC_FOLD: "4-wide partials + fold", PARTS: "from parts"}


def _G():
    import gpu_util as G
    return G


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---------------------------------------------------------------- launch shapes (host mirrors of bn_split / pick_rsplit / bnmap in losses.hip)
def vec_split(rows):
    """(blocks, rows per block) of the 4-wide kernels for rows <= 16 x 8 x CUs (every case here): at most one block per 16 rows"""
    want = max(1, (rows + 15) // 16)
    rpb = -(-rows // want)
    return -(-rows // rpb), rpb


def scalar_split(rows, det):
    """(row splits, rows per split) of the scalar kernels for rows <= 64 x 8 x CUs / ceil(C / 64): one split per 64 rows, one in deterministic mode"""
    want = 1 if det else max(1, (rows + 63) // 64)
    rpb = -(-rows // want)
    return -(-rows // rpb), rpb


def vec_map(C):
    tx = min(C // 4, 256)
    return tx, 256 // tx


def expected_route(rows, C, ld_ok, det, mode, backward):
    """the route record a case must report, from its shape alone"""
    if mode == "plain":
        stats = NONE
    elif mode == "eval":
        stats = EVAL
    elif C % 4 == 0 and ld_ok and C <= 1024:
        stats = VEC_FOLD if (det or backward) else VEC_FF
    else:
        stats = SCALAR
    r = dict(stats=stats, apply=1 if (C % 4 == 0 and ld_ok) else 0, det=1 if det else 0, blocks=0, rpb=0, tx=0, ty=0)
    if stats in (VEC_FF, VEC_FOLD):
        r["blocks"], r["rpb"] = vec_split(rows); r["tx"], r["ty"] = vec_map(C)
    elif stats == SCALAR:
        r["blocks"], r["rpb"] = scalar_split(rows, det); r["tx"], r["ty"] = 64, 4
    return r


def stats_n_p(route):
    """(n_p, block partial rounded to fp32) of the statistics launch"""
    if route["stats"] in (VEC_FF, VEC_FOLD):
        return -(-route["rpb"] // route["ty"]), True
    return -(-route["rpb"] // 4) + 3, False


def _route(G_, backward):
    out = (ctypes.c_int * 8)()
    G_.check(G_.lib.eegldm_debug_bn_last_route(backward, out))
    return dict(stats=out[0], apply=out[1], blocks=out[2], rpb=out[3], tx=out[4], ty=out[5], det=out[6], apply_rpb=out[7])


def _confirm(G_, backward, want, tag):
    got = _route(G_, backward)
    for k, v in want.items():
        assert got[k] == v, f"{tag}: {'backward' if backward else 'forward'} served by {FAMILY.get(got['stats'], got['stats'])} {got}, expected {k} = {v}"
    print(f"[route] {tag} {'bwd' if backward else 'fwd'}: statistics {FAMILY[got['stats']]}, apply {'4-wide' if got['apply'] else 'scalar'}, blocks={got['blocks']} "
          f"rows/block={got['rpb']} TX={got['tx']} TY={got['ty']} det={got['det']}")


# ---------------------------------------------------------------- BatchNorm cases
# name, (B, L, C), ld ("C", "2C" or a number), dtypes, offsets (sigma; bf16 skips 100), scale, mode ("train" / "eval" / "plain"), options
#   options: "det" deterministic mode (two runs must be bit-equal), "acc" dgamma / dbeta start from non-zero values
ALL = (0, 1, 2)
BN_CASES = [
    ("4-wide fold_finalize", (2, 200, 64), "C", ALL, (0.0, 30.0, 100.0), 1.0, "train", "acc"),
    ("4-wide ordered fold (deterministic)", (2, 200, 64), "C", ALL, (0.0, 30.0, 100.0), 1.0, "train", "det"),
    ("4-wide C12 (TX 3, TY 85)", (2, 50, 12), "C", ALL, (30.0,), 1.0, "train", "acc"),
    ("4-wide C516 (TX 129, TY 1)", (2, 24, 516), "C", ALL, (30.0,), 1.0, "train", ""),
    ("4-wide C1024 (TX 256)", (2, 24, 1024), "C", ALL, (0.0,), 1.0, "train", "acc"),
    ("scalar statistics + 4-wide apply C1028", (2, 24, 1028), "C", ALL, (30.0,), 1.0, "train", ""),
    ("scalar odd C6", (2, 50, 6), "C", ALL, (30.0,), 1.0, "train", "acc"),
    ("scalar via ld 10", (2, 50, 8), 10, ALL, (0.0,), 1.0, "train", ""),
    ("4-wide column view ld 2C", (2, 100, 64), "2C", ALL, (30.0,), 1.0, "train", "acc"),
    ("scalar deterministic (one block, 300 rows)", (3, 100, 6), "C", ALL, (30.0,), 1.0, "train", "det"),
    ("few rows (1, 2, 64)", (1, 2, 64), "C", ALL, (0.0,), 1.0, "train", ""),
    ("few rows (2, 9, 64)", (2, 9, 64), "C", ALL, (30.0,), 1.0, "train", "acc"),
    ("eps matters: |x| 1e-3", (2, 200, 64), "C", ALL, (0.0,), 1e-3, "train", ""),
    ("range: |x| 100", (2, 200, 64), "C", ALL, (0.0,), 100.0, "train", "acc"),
    ("eval C64", (2, 50, 64), "C", ALL, (30.0,), 1.0, "eval", ""),
    ("eval C6", (2, 50, 6), "C", ALL, (0.0,), 1.0, "eval", ""),
    ("plain LeakyReLU C64", (2, 50, 64), "C", ALL, (0.0,), 1.0, "plain", ""),
    ("plain LeakyReLU C6", (2, 50, 6), "C", ALL, (0.0,), 1.0, "plain", ""),
]


def case_runs(case):
    """(dt, offset) pairs of a case: bf16 is not used at 100 sigma (module docstring)"""
    return [(dt, off) for dt in case[3] for off in case[4] if not (dt == 1 and off >= 100.0)]


def case_ld(case):
    C = case[1][2]
    return C if case[2] == "C" else (2 * C if case[2] == "2C" else int(case[2]))


def bn_inputs(case, dt, off, poison=None):
    """the operands of a case, as float64 tensors holding storage values: x, dy (rows, C); gamma (every third channel negative), beta;
    running statistics and accumulated-gradient start values.  Seeds are fixed: the CPU test rebuilds exactly these."""
    _name, (B, L, C), _ld, _dts, _offs, scale, mode, opts = case
    fmt = FMT[dt]
    rows = B * L
    x = N.to_storage(scale * (_randn((rows, C), 171) + off), fmt)
    if poison:
        for (r, c), v in poison:
            x[r, c] = v
    else:
        assert bool(torch.isfinite(x).all()), f"{case[0]} [{fmt}]: non-finite input"
    sign = torch.where(torch.arange(C) % 3 == 2, -1.0, 1.0).double()
    ga = N.rne(sign * (1 + 0.1 * _randn((C,), 172)), "f32"); be = N.rne(0.1 * _randn((C,), 173), "f32")
    dy = N.to_storage(_randn((rows, C), 174), fmt)
    rm = N.rne(scale * (off + 0.1 * _randn((C,), 175)), "f32"); rv = N.rne(scale * scale * (1 + 0.1 * _randn((C,), 176).abs()), "f32")
    acc = "acc" in opts
    dg0 = N.rne(_randn((C,), 177), "f32") if acc else torch.zeros(C, dtype=torch.float64)
    db0 = N.rne(_randn((C,), 178), "f32") if acc else torch.zeros(C, dtype=torch.float64)
    return dict(x=x, ga=ga, be=be, dy=dy, rm=rm, rv=rv, nbt=3.0, dg0=dg0, db0=db0, fmt=fmt, mode=mode, rows=rows, C=C)


def bn_reference(inp, route_f):
    """Everything that is known before the kernel runs: float64 references, bounds and the mask-uncertain set, whose share is asserted here."""
    x, ga, be, fmt, mode = inp["x"], inp["ga"], inp["be"], inp["fmt"], inp["mode"]
    u = N.U32
    ref = dict(mode=mode)
    if mode == "plain":
        ref["y"] = N.rne((x.float() * np.float32(SLOPE)).double(), fmt)            # the fp32 product, rounded once to the storage type
        ref["y"] = torch.where(x > 0, x, ref["y"])
        dyp = N.rne((inp["dy"].float() * np.float32(SLOPE)).double(), fmt)
        ref["dx"] = torch.where(x > 0, inp["dy"], dyp)
        return ref
    if mode == "eval":
        st = dict(mean=inp["rm"].clone(), var=inp["rv"].clone(), rstd=1.0 / torch.sqrt(inp["rv"] + EPS))
        e_mean, e_rstd = torch.zeros_like(st["mean"]), torch.full_like(st["mean"], 4 * u)
    else:
        st = N.bn_stats(x, EPS, inp["rm"], inp["rv"], inp["nbt"])
        n_p, blk = stats_n_p(route_f)
        e_mean, e_rstd = N.bn_stat_bounds(x, st, n_p, blk, EPS)
        n = inp["rows"]
        ub = st["var"] * n / max(n - 1, 1)
        e_var = (e_rstd - 4 * u) * 2 * (st["var"] + EPS)
        ref["b_rm"] = 0.1 * e_mean + 4 * u * (0.9 * inp["rm"].abs() + 0.1 * st["mean"].abs())
        ref["b_rv"] = 0.1 * (e_var + u * st["var"]) * n / max(n - 1, 1) + 4 * u * (0.9 * inp["rv"].abs() + 0.1 * ub)
    z, y, d = N.bn_fwd_bound(x, ga, be, st, e_mean, e_rstd, SLOPE)
    ref.update(st=st, e_mean=e_mean, e_rstd=e_rstd, z=z, y=y, d=d)
    if fmt != "f32":
        xe = x.float()
        if mode == "eval":
            ze = F.batch_norm(xe, inp["rm"].float(), inp["rv"].float(), ga.float(), be.float(), False, 0.1, EPS)
        else:
            ze = F.batch_norm(xe, None, None, ga.float(), be.float(), True, 0.1, EPS)
        ref["y_emul"] = F.leaky_relu(ze, SLOPE)
    if mode == "train":
        b = N.bn_bwd_bounds(x, ga, be, st, e_mean, e_rstd, inp["dy"], SLOPE, d, dgamma0=inp["dg0"], dbeta0=inp["db0"])
        ref["bwd"] = b
        fin = torch.isfinite(z)
        share = float((b["U"] & fin).double().sum() / max(1, int(fin.sum())))
        ref["share"] = share
        assert share <= U_CAP, f"mask-uncertain share {share:.3e} above {U_CAP}: the case needs other inputs"
        if fmt != "f32":
            xr = x.float().requires_grad_(True)
            ye = F.leaky_relu(F.batch_norm(xr, None, None, ga.float(), be.float(), True, 0.1, EPS), SLOPE)
            (ref["dx_emul"],) = torch.autograd.grad(ye, xr, inp["dy"].float())
    return ref


def _nanmax(t):
    t = t[torch.isfinite(t)]
    return float(t.max()) if t.numel() else float("nan")


def bn_judge(got, inp, ref, tag):
    """Hold a result (from the device, or from the CPU model of the kernels) to the reference: got = dict(st (C, 2), y, rm, rv, nbt and, for
    the training cases, dx, dga, dbe).  Returns the list of failed checks (name, message); prints one [numerics] line per check."""
    fmt, mode = inp["fmt"], inp["mode"]
    fails = []

    def run(name, fn):
        try:
            fn()
        except AssertionError as e:
            fails.append((name, str(e)))

    if mode == "plain":
        for k in ("y", "dx"):
            def exact(k=k):
                bad = ~N._same(N._f64(got[k]), ref[k])
                print(f"[numerics] {tag} {k}: {int(bad.sum())} of {bad.numel()} differ from the exact result")
                assert not bool(bad.any()), f"{tag} {k}: {int(bad.sum())} elements differ from the exact result"
            run(k, exact)
        return fails
    st, e_mean, e_rstd = ref["st"], ref["e_mean"], ref["e_rstd"]

    def stats():
        m, r = N._f64(got["st"][:, 0]), N._f64(got["st"][:, 1])
        nan_ok = bool((torch.isnan(m) == torch.isnan(st["mean"])).all()) and bool((torch.isnan(r) == torch.isnan(st["rstd"])).all()) \
            and bool((m[torch.isinf(st["mean"])] == st["mean"][torch.isinf(st["mean"])]).all())
        fin = torch.isfinite(st["mean"]) & torch.isfinite(st["rstd"])
        em = (m - st["mean"]).abs()[fin]; er = (r / st["rstd"] - 1).abs()[fin]
        bm, br = e_mean[fin], e_rstd[fin]
        rm_ = torch.where(em == 0, torch.zeros_like(em), em / bm); rr_ = er / br
        print(f"[numerics] {tag} stats: e_mean {_nanmax(em * st['rstd'][fin]):.2e} sigma (bound {_nanmax(bm * st['rstd'][fin]):.2e}) = {_nanmax(rm_):.3f} x bound, "
              f"e_rstd {_nanmax(er):.2e} (bound {_nanmax(br):.2e}) = {_nanmax(rr_):.3f} x bound, mean^2 / var up to {_nanmax((st['mean'] ** 2 / st['var'])[fin]):.3g}")
        assert nan_ok, f"{tag}: non-finite pattern of the statistics differs from the reference"
        assert bool((rm_ <= 1).all()) and bool((rr_ <= 1).all()), f"{tag}: statistics outside their bound (mean {_nanmax(rm_):.3g} x, rstd {_nanmax(rr_):.3g} x)"
    run("stats", stats)
    run("y A", lambda: N.check_abs(got["y"], ref["y"], ref["d"], fmt, route=tag + " fwd A"))
    if fmt != "f32" and bool(torch.isfinite(ref["y"]).all()):
        run("y B", lambda: N.check_b(got["y"], ref["y"], ref["y_emul"], fmt, route=tag + " fwd B"))
    if mode == "eval":
        def untouched():
            assert torch.equal(N._f64(got["rm"]), inp["rm"]) and torch.equal(N._f64(got["rv"]), inp["rv"]) and float(got["nbt"]) == inp["nbt"], \
                f"{tag}: eval mode changed the running statistics"
            print(f"[numerics] {tag}: running statistics and num_batches_tracked untouched")
        run("running", untouched)
        return fails
    run("running mean", lambda: N.check_abs(got["rm"], st["rmean"], ref["b_rm"], "f32", route=tag + " running mean"))
    run("running var", lambda: N.check_abs(got["rv"], st["rvar"], ref["b_rv"], "f32", route=tag + " running var"))

    def nbt():
        assert float(got["nbt"]) == st["nbt"], f"{tag}: num_batches_tracked {float(got['nbt'])}, expected {st['nbt']}"
    run("nbt", nbt)
    if "dx" not in got:
        return fails
    b = ref["bwd"]
    print(f"[numerics] {tag} mask-uncertain share {ref['share']:.2e} (cap {U_CAP})")
    run("dx A", lambda: N.check_abs(got["dx"], b["dx"], b["b_dx"], fmt, route=tag + " dx A", alt=(b["dx_alt"], b["U"])))
    if fmt != "f32" and bool(torch.isfinite(b["dx"]).all()):
        run("dx B", lambda: N.check_b(got["dx"], b["dx"], ref["dx_emul"], fmt, route=tag + " dx B"))
    run("dbeta", lambda: N.check_abs(got["dbe"], b["dbeta"], b["b_dbeta"], "f32", route=tag + " dbeta"))
    run("dgamma", lambda: N.check_abs(got["dga"], b["dgamma"], b["b_dgamma"], "f32", route=tag + " dgamma"))
    return fails


def _dev_rows(G_, t, ld, dt, pad=1.0e4):
    """(rows, C) float64 storage values -> device [rows, ld] of the engine dtype; the columns outside the view hold a finite junk value
    that would wreck the statistics if a kernel read them"""
    rows, C = t.shape
    buf = torch.full((rows, ld), pad, dtype=G_.TDT[dt])
    buf[:, :C] = t.to(G_.TDT[dt])
    return buf.to(G_.DEV)


def _out_rows(G_, rows, C, ld, dt):
    return torch.full((rows, ld), math.nan, device=G_.DEV, dtype=G_.TDT[dt])


def _read_rows(buf, C, tag):
    """the [rows, C] view as float64; the columns outside the view must still hold their NaN fill"""
    assert bool(torch.isnan(buf[:, C:]).all()), f"{tag}: wrote outside the [rows, C] view"
    return buf[:, :C].double().cpu()


def bn_run(G_, c, case, dt, inp, env_switches, tag, ref=None, stats_from_ref=False):
    """forward (+ backward for the training cases) on the device with route confirmation; returns the `got` dict of bn_judge"""
    _name, (B, L, C), _ld, _dts, _offs, _scale, mode, opts = case
    rows, ld = B * L, case_ld(case)
    det = "det" in opts
    env_switches(EEGLDM_DETERMINISTIC="1" if det else None)
    ld_ok = ld % 4 == 0
    want_f = expected_route(rows, C, ld_ok, det, mode, 0)
    xd = _dev_rows(G_, inp["x"], ld, dt)
    f32 = lambda t: t.float().to(G_.DEV)
    gad, bed = f32(inp["ga"]), f32(inp["be"])
    rm, rv, nbt = f32(inp["rm"]), f32(inp["rv"]), torch.full((1,), inp["nbt"], device=G_.DEV)
    st = torch.full((C, 2), math.nan, device=G_.DEV)
    yb = _out_rows(G_, rows, C, ld, dt)
    plain = mode == "plain"
    G_.check(G_.lib.eegldm_batchnorm_lrelu_fwd(c.h, G_.ptr(xd), ld, None if plain else G_.ptr(gad), None if plain else G_.ptr(bed),
                                               None if plain else G_.ptr(st), None if plain else G_.ptr(rm), None if plain else G_.ptr(rv),
                                               None if plain else G_.ptr(nbt), G_.ptr(yb), ld, rows, C, SLOPE, 0 if mode == "eval" else 1, dt))
    torch.cuda.synchronize()
    _confirm(G_, 0, want_f, tag)
    got = dict(st=st.cpu().double(), y=_read_rows(yb, C, tag + " y"), rm=rm.cpu().double(), rv=rv.cpu().double(), nbt=float(nbt))
    if mode == "eval":
        return got
    want_b = expected_route(rows, C, ld_ok, det, mode, 1)
    dyd = _dev_rows(G_, inp["dy"], ld, dt)
    runs = []
    for _rep in range(2 if det else 1):
        dxb = _out_rows(G_, rows, C, ld, dt)
        dga, dbe = f32(inp["dg0"]), f32(inp["db0"])
        G_.check(G_.lib.eegldm_batchnorm_lrelu_bwd(c.h, G_.ptr(xd), ld, None if plain else G_.ptr(gad), None if plain else G_.ptr(bed),
                                                   None if plain else G_.ptr(st), G_.ptr(dyd), ld, G_.ptr(dxb), ld,
                                                   None if plain else G_.ptr(dga), None if plain else G_.ptr(dbe), rows, C, SLOPE, dt))
        torch.cuda.synchronize()
        _confirm(G_, 1, want_b, tag)
        runs.append(dict(dx=_read_rows(dxb, C, tag + " dx"), dga=dga.cpu().double(), dbe=dbe.cpu().double()))
    got.update(runs[0])
    if det:
        for k in ("dx", "dga", "dbe"):
            assert N._same(runs[0][k], runs[1][k]).all(), f"{tag}: {k} differs between two deterministic-mode runs"
        print(f"[numerics] {tag}: dx, dgamma, dbeta bit-equal across two deterministic-mode runs")
    env_switches(EEGLDM_DETERMINISTIC=None)
    return got


def _ids(cases):
    return [c[0] for c in cases]


def _raise(fails):
    assert not fails, "; ".join(f"[{n}] {m}" for n, m in fails)


@pytest.mark.parametrize("case", BN_CASES, ids=_ids(BN_CASES))
def test_batchnorm_route_against_float64(case, env_switches):
    G_ = _G(); c = G_.ctx()
    _name, (B, L, C), _ld, _dts, _offs, _scale, mode, opts = case
    fails = []
    for dt, off in case_runs(case):
        tag = f"{case[0]} [{FMT[dt]}, mean {off:g} sigma]"
        inp = bn_inputs(case, dt, off)
        ref = bn_reference(inp, expected_route(B * L, C, case_ld(case) % 4 == 0, "det" in opts, mode, 0))     # the U cap is asserted in here
        got = bn_run(G_, c, case, dt, inp, env_switches, tag)
        fails += bn_judge(got, inp, ref, tag)
    _raise(fails)


NONFINITE = [c for c in BN_CASES if c[0] in ("4-wide fold_finalize", "scalar odd C6")]


@pytest.mark.parametrize("case", NONFINITE, ids=_ids(NONFINITE))
def test_nonfinite_stays_in_its_channel(case, env_switches):
    """One NaN in x (channel 1) and one inf (channel C - 2) must make those channels' statistics and whole outputs non-finite exactly as in
    float64 and leave every other channel inside its bounds; the same for a NaN in dy through the backward (dx, dgamma, dbeta of that channel)."""
    G_ = _G(); c = G_.ctx()
    _name, (B, L, C), _ld, _dts, _offs, _scale, mode, opts = case
    fails = []
    for dt in (0, 1):
        tag = f"{case[0]} non-finite [{FMT[dt]}]"
        inp = bn_inputs(case, dt, 0.0, poison=[((7, 1), math.nan), ((B * L - 3, C - 2), math.inf)])
        inp["dy"][11, 3] = math.nan
        ref = bn_reference(inp, expected_route(B * L, C, True, False, mode, 0))
        for k, ch in (("y", (1, C - 2)), ("dx", (1, 3, C - 2))):
            r = ref[k] if k == "y" else ref["bwd"][k]
            bad = ~torch.isfinite(r)
            assert bool(bad[:, list(ch)].all()) and int(bad.sum()) == len(ch) * B * L, f"{tag}: the reference's non-finite pattern of {k} is not the poisoned channels"
        got = bn_run(G_, c, case, dt, inp, env_switches, tag)
        fails += bn_judge(got, inp, ref, tag)
        print(f"[nonfinite] {tag}: y non-finite in channels 1 and {C - 2}, dx also in channel 3, every other channel inside its bounds")
    _raise(fails)


# ---------------------------------------------------------------- statistics from host-made partials
PARTS_SIZES = [(1, 2), (15, 32), (16, 32), (17, 34), (2048, 64)]


def parts_inputs(nparts, C, rows_per_part=4):
    """fp32 partials [nparts][2 C] of a data set whose odd channels have mean^2 / var = 1e4 (mean 100, sigma 1); rows = nparts x rows_per_part"""
    n = nparts * rows_per_part
    mean = torch.where(torch.arange(C) % 2 == 1, 100.0, 0.3).double()
    x = _randn((n, C), 181) + mean
    xb = x.reshape(nparts, rows_per_part, C)
    parts = torch.stack([xb.sum(1), (xb * xb).sum(1)], dim=-1).reshape(nparts, 2 * C)       # interleaved (sum, sum of squares)
    parts = N.rne(parts, "f32")
    rm = N.rne(0.1 * _randn((C,), 182), "f32"); rv = N.rne(1 + 0.1 * _randn((C,), 183).abs(), "f32")
    return dict(parts=parts, n=n, C=C, nparts=nparts, rm=rm, rv=rv, nbt=5.0)


def parts_reference(pi):
    p = pi["parts"].numpy(); C, n, nparts = pi["C"], pi["n"], pi["nparts"]
    S = torch.tensor([math.fsum(p[:, j]) for j in range(2 * C)], dtype=torch.float64).reshape(C, 2)
    st = N.bn_stats_from_sums(S[:, 0], S[:, 1], n, EPS)
    u = N.U32
    e_mean = u * st["mean"].abs()
    amp = (st["var"] + st["mean"] ** 2) / (st["var"] + EPS)
    e_rstd = N.gamma64(nparts) * amp + 4 * u
    ub = st["var"] * n / max(n - 1, 1)
    rmean = 0.9 * pi["rm"] + 0.1 * st["mean"]; rvar = 0.9 * pi["rv"] + 0.1 * ub
    e_var = 2 * N.gamma64(nparts) * (st["var"] + st["mean"] ** 2)
    return dict(st=st, e_mean=e_mean, e_rstd=e_rstd, amp=amp, rmean=rmean, rvar=rvar,
                b_rm=0.1 * e_mean + 4 * u * (0.9 * pi["rm"].abs() + 0.1 * st["mean"].abs()),
                b_rv=0.1 * (e_var + u * st["var"]) * n / max(n - 1, 1) + 4 * u * (0.9 * pi["rv"].abs() + 0.1 * ub))


def parts_judge(got, pi, ref, tag):
    fails = []
    st = ref["st"]
    m, r = N._f64(got["st"][:, 0]), N._f64(got["st"][:, 1])
    em = (m - st["mean"]).abs(); er = (r / st["rstd"] - 1).abs()
    rm_ = torch.where(em == 0, torch.zeros_like(em), em / ref["e_mean"]); rr_ = er / ref["e_rstd"]
    print(f"[numerics] {tag} stats: e_mean {float(rm_.max()):.3f} x bound, e_rstd {float(er.max()):.2e} (bound {float(ref['e_rstd'].max()):.2e}) = {float(rr_.max()):.3f} x bound, "
          f"(var + mean^2) / (var + eps) up to {float(ref['amp'].max()):.3g}")
    if not (bool((rm_ <= 1).all()) and bool((rr_ <= 1).all())):
        fails.append(("stats", f"{tag}: statistics outside their bound (mean {float(rm_.max()):.3g} x, rstd {float(rr_.max()):.3g} x)"))
    for k, rk, bk in (("rm", "rmean", "b_rm"), ("rv", "rvar", "b_rv")):
        try:
            N.check_abs(got[k], ref[rk], ref[bk], "f32", route=f"{tag} running {'mean' if k == 'rm' else 'var'}")
        except AssertionError as e:
            fails.append((k, str(e)))
    if float(got["nbt"]) != pi["nbt"] + 1:
        fails.append(("nbt", f"{tag}: num_batches_tracked {float(got['nbt'])}"))
    return fails


@pytest.mark.parametrize("det", [0, 1], ids=["fold_finalize", "ordered fold + finalize"])
@pytest.mark.parametrize("size", PARTS_SIZES, ids=[f"{n}x{c}" for n, c in PARTS_SIZES])
def test_statistics_from_parts(size, det, env_switches):
    G_ = _G(); c = G_.ctx()
    env_switches(EEGLDM_DETERMINISTIC="1" if det else None)
    pi = parts_inputs(*size)
    ref = parts_reference(pi)
    tag = f"from parts {size[0]} x {size[1]}{' deterministic' if det else ''}"
    pd = pi["parts"].float().to(G_.DEV)
    st = torch.full((pi["C"], 2), math.nan, device=G_.DEV)
    rm, rv, nbt = pi["rm"].float().to(G_.DEV), pi["rv"].float().to(G_.DEV), torch.full((1,), pi["nbt"], device=G_.DEV)
    G_.check(G_.lib.eegldm_debug_bn_stats_from_parts(c.h, G_.ptr(pd), pi["nparts"], G_.ptr(st), G_.ptr(rm), G_.ptr(rv), G_.ptr(nbt), pi["n"], pi["C"]))
    torch.cuda.synchronize()
    _confirm(G_, 0, dict(stats=PARTS, blocks=pi["nparts"], det=det), tag)
    _raise(parts_judge(dict(st=st.cpu().double(), rm=rm.cpu().double(), rv=rv.cpu().double(), nbt=float(nbt)), pi, ref, tag))


# ---------------------------------------------------------------- fused tail
def tail_shape(C, dt):
    """(G, NJ) of the template instantiation, None when the channel count is not eligible (tail_shape in disc_tail.hip)"""
    E = 4 if dt == 0 else 8
    if C % E:
        return None
    ch = C // E
    if ch >= 64:
        return (64, ch // 64) if ch % 64 == 0 and ch // 64 <= 2 else None
    return (ch, 1) if ch in (4, 8, 16, 32) else None


def tail_inputs(B, L, C, dt, bias=True, acc=True, seed=191):
    fmt = FMT[dt]
    y = N.to_storage(1.5 * _randn((B, L, C), seed) + 0.4, fmt)
    sign = torch.where(torch.arange(C) % 3 == 2, -1.0, 1.0).double()
    ga = N.rne(sign * (1 + 0.1 * _randn((C,), seed + 1)), "f32"); be = N.rne(0.1 * _randn((C,), seed + 2), "f32")
    w3 = N.rne(_randn((3, C), seed + 3) / math.sqrt(3 * C), "f32")
    b = N.rne(0.3 * _randn((1,), seed + 4), "f32") if bias else None
    dl = N.rne(_randn((B, L), seed + 5), "f32")
    z = torch.zeros
    start = dict(dga=N.rne(_randn((C,), seed + 6), "f32") if acc else z(C).double(), dbe=N.rne(_randn((C,), seed + 7), "f32") if acc else z(C).double(),
                 dw3=N.rne(_randn((3, C), seed + 8), "f32") if acc else z(3, C).double(), dbias=N.rne(_randn((1,), seed + 9), "f32") if acc else z(1).double())
    return dict(y=y, ga=ga, be=be, w3=w3, bias=b, dl=dl, start=start, fmt=fmt, B=B, L=L, C=C)


def tail_reference(ti, st=None, e_mean=None, e_rstd=None):
    """references, bounds and the U cap for the fused tail; st: the statistics the kernel is handed (default: float64 ones, which the caller
    rounds to fp32: e_mean = u |mean|, e_rstd = u)"""
    y, ga, be, w3, dl, fmt = ti["y"], ti["ga"], ti["be"], ti["w3"], ti["dl"], ti["fmt"]
    B, L, C = y.shape; rows = B * L
    u = N.U32
    y2 = y.reshape(rows, C)
    if st is None:
        st = N.bn_stats(y2, EPS)
        e_mean, e_rstd = u * st["mean"].abs(), torch.full_like(st["mean"], u)
    z, a, d = N.bn_fwd_bound(y2, ga, be, st, e_mean, e_rstd, SLOPE)
    a3, d3 = a.reshape(B, L, C), d.reshape(B, L, C)
    ref = dict(st=st)
    ref["logits"] = N.tail_logits(y, ga, be, st, w3, ti["bias"], SLOPE)
    wabs = w3.abs()
    spread = N.tail_logits(y, None, None, None, wabs, None, SLOPE, a=d3)
    ref["b_logits"] = N.gamma(3 * C + 4) * (N.tail_logits(y, None, None, None, wabs, None, SLOPE, a=a3.abs() + d3) + (abs(float(ti["bias"])) if ti["bias"] is not None else 0.0)) + spread
    da = N.tail_da(dl, w3).reshape(rows, C); da_mag = N.tail_da(dl.abs(), wabs).reshape(rows, C)
    s0 = ti["start"]
    b = N.bn_bwd_bounds(y2, ga, be, st, e_mean, e_rstd, da, SLOPE, d, da_mag=da_mag, k_da=3, dgamma0=s0["dga"], dbeta0=s0["dbe"])
    ref["bwd"] = b; ref["share"] = b["share"]
    assert b["share"] <= U_CAP, f"mask-uncertain share {b['share']:.3e} above {U_CAP}: the case needs other inputs"
    dlt = [N._shift_rows(dl, 1 - t)[:, :, None] for t in range(3)]
    ref["dw3"] = torch.stack([(a3 * dlt[t]).sum((0, 1)) for t in range(3)]) + s0["dw3"]
    ref["b_dw3"] = torch.stack([N.gamma(rows + 2) * (((a3.abs() + d3) * dlt[t].abs()).sum((0, 1)) + s0["dw3"][t].abs()) + (d3 * dlt[t].abs()).sum((0, 1)) for t in range(3)])
    ref["dbias"] = dl.sum().reshape(1) + s0["dbias"]
    ref["b_dbias"] = N.gamma(rows) * (dl.abs().sum().reshape(1) + s0["dbias"].abs())
    if fmt != "f32":
        yr = y.float().permute(0, 2, 1).contiguous().requires_grad_(True)                     # NCL for torch
        ae = F.leaky_relu(F.batch_norm(yr, None, None, ga.float(), be.float(), True, 0.1, EPS), SLOPE)
        lg = F.conv1d(ae, w3.float().t().reshape(1, C, 3), None, padding=1)
        (g,) = torch.autograd.grad(lg, yr, dl.float().reshape(B, 1, L))
        ref["dy_emul"] = g.permute(0, 2, 1).reshape(rows, C)
    return ref


def tail_judge(got, ti, ref, tag):
    """got: logits (B, L), dy (rows, C), dga, dbe, dw3 (3, C), dbias (1,) -- any subset"""
    fmt = ti["fmt"]; b = ref["bwd"]
    fails = []

    def run(name, fn):
        try:
            fn()
        except AssertionError as e:
            fails.append((name, str(e)))

    if "logits" in got:
        run("logits", lambda: N.check_abs(got["logits"], ref["logits"], ref["b_logits"], "f32", route=tag + " logits"))
    if "dy" in got:
        print(f"[numerics] {tag} mask-uncertain share {ref['share']:.2e} (cap {U_CAP})")
        run("dy A", lambda: N.check_abs(got["dy"], b["dx"], b["b_dx"], fmt, route=tag + " dy A", alt=(b["dx_alt"], b["U"])))
        if fmt != "f32":
            run("dy B", lambda: N.check_b(got["dy"], b["dx"], ref["dy_emul"], fmt, route=tag + " dy B"))
    if "dga" in got:
        run("dbeta", lambda: N.check_abs(got["dbe"], b["dbeta"], b["b_dbeta"], "f32", route=tag + " dbeta"))
        run("dgamma", lambda: N.check_abs(got["dga"], b["dgamma"], b["b_dgamma"], "f32", route=tag + " dgamma"))
    if "dw3" in got:
        run("dw3", lambda: N.check_abs(got["dw3"], ref["dw3"], ref["b_dw3"], "f32", route=tag + " dw3"))
        run("dbias", lambda: N.check_abs(got["dbias"], ref["dbias"], ref["b_dbias"], "f32", route=tag + " dbias"))
    return fails


def tail_run(G_, c, ti, dt, tag, st_dev=None, ld=None, fwd=True, bwd=True, pg=True):
    B, L, C = ti["B"], ti["L"], ti["C"]; rows = B * L
    ld = ld or C
    f32 = lambda t: t.float().to(G_.DEV)
    yd = _dev_rows(G_, ti["y"].reshape(rows, C), ld, dt)
    gad, bed, w3d = f32(ti["ga"]), f32(ti["be"]), f32(ti["w3"]).contiguous()
    bd = f32(ti["bias"]) if ti["bias"] is not None else None
    if st_dev is None:
        st = N.bn_stats(ti["y"].reshape(rows, C), EPS)
        st_dev = torch.stack([st["mean"], st["rstd"]], dim=1).float().to(G_.DEV).contiguous()
    G_n, NJ = tail_shape(C, dt)
    got = {}
    if fwd:
        lg = torch.full((B, L), math.nan, device=G_.DEV)
        G_.check(G_.lib.eegldm_debug_disc_tail_fwd(c.h, dt, G_.ptr(yd), ld, G_.ptr(gad), G_.ptr(bed), G_.ptr(st_dev), G_.ptr(w3d), G_.ptr(bd), SLOPE, G_.ptr(lg), B, L, C))
        torch.cuda.synchronize()
        print(f"[route] {tag} fwd: tail_fwd_kernel<{FMT[dt]}, G={G_n}, NJ={NJ}> rblk={min(16, L)} ld={ld}")
        got["logits"] = lg.cpu().double()
    if bwd:
        dld = f32(ti["dl"]).contiguous()
        dyb = _out_rows(G_, rows, C, ld, dt)
        s0 = ti["start"]
        dga, dbe, dw3, dbias = (f32(s0[k]).contiguous() for k in ("dga", "dbe", "dw3", "dbias"))
        P = (lambda t: G_.ptr(t)) if pg else (lambda t: None)
        G_.check(G_.lib.eegldm_debug_disc_tail_bwd(c.h, dt, G_.ptr(yd), ld, G_.ptr(gad), G_.ptr(bed), G_.ptr(st_dev), G_.ptr(w3d), SLOPE, G_.ptr(dld), G_.ptr(dyb), ld,
                                                   P(dga), P(dbe), P(dw3), P(dbias), B, L, C))
        torch.cuda.synchronize()
        print(f"[route] {tag} bwd: tail_bwd_reduce / apply<{FMT[dt]}, G={G_n}, NJ={NJ}, PG={'true' if pg else 'false'}> ld={ld} "
              f"det={1 if os.environ.get('EEGLDM_DETERMINISTIC') else 0}")
        got["dy"] = _read_rows(dyb, C, tag + " dy")
        if pg:
            got.update(dga=dga.cpu().double(), dbe=dbe.cpu().double(), dw3=dw3.cpu().double(), dbias=dbias.cpu().double())
        else:
            for k, t in (("dga", dga), ("dbe", dbe), ("dw3", dw3), ("dbias", dbias)):
                assert torch.equal(t.cpu().double(), s0[k]), f"{tag}: {k} changed although no parameter gradients were asked for"
    return got


TAIL_C = {0: (16, 32, 64, 128, 256, 512), 1: (32, 64, 128, 256, 512, 1024), 2: (32, 64, 128, 256, 512, 1024)}


@pytest.mark.parametrize("L", [37, 8])
@pytest.mark.parametrize("dt", [0, 1, 2], ids=["f32", "bf16", "f16"])
def test_fused_tail_every_instantiation(dt, L, env_switches):
    """B = 3; L = 37: rblk clamped to 16, last block short, halo rows at both sample ends; L = 8: rblk > L and L < 4 RPW for G <= 16 (the
    backward's row walk wraps a sample within one step)"""
    G_ = _G(); c = G_.ctx()
    fails = []
    for C in TAIL_C[dt]:
        tag = f"tail C{C} L{L} [{FMT[dt]}]"
        ti = tail_inputs(3, L, C, dt)
        ref = tail_reference(ti)
        fails += tail_judge(tail_run(G_, c, ti, dt, tag), ti, ref, tag)
    _raise(fails)


@pytest.mark.parametrize("dt", [0, 1, 2], ids=["f32", "bf16", "f16"])
def test_fused_tail_options(dt, env_switches):
    """at C = 64: a column view (ldy = 2 C), no bias, the backward without parameter gradients (dy bit-equal to the full run's, gradient
    buffers untouched), statistics taken from eegldm_batchnorm_lrelu_fwd (the composition eegldm_disc_forward runs), and refusals"""
    G_ = _G(); c = G_.ctx()
    C, B, L = 64, 3, 37
    fails = []
    ti = tail_inputs(B, L, C, dt, bias=False, acc=False)
    ref = tail_reference(ti)
    tag = f"tail C{C} ld 2C, no bias [{FMT[dt]}]"
    full = tail_run(G_, c, ti, dt, tag, ld=2 * C)
    fails += tail_judge(full, ti, ref, tag)
    nopg = tail_run(G_, c, ti, dt, tag + " PG=false", ld=2 * C, fwd=False, pg=False)
    assert N._same(nopg["dy"], full["dy"]).all(), f"{tag}: dy of the backward without parameter gradients differs from the full backward's"
    print(f"[numerics] {tag}: dy bit-equal with and without parameter gradients")
    # statistics from the BatchNorm forward: the tail inherits that route's statistics error
    tag = f"tail C{C} statistics from batchnorm_lrelu_fwd [{FMT[dt]}]"
    ti = tail_inputs(B, L, C, dt, seed=291)
    rows = B * L
    y2 = ti["y"].reshape(rows, C)
    route_f = expected_route(rows, C, True, False, "train", 0)
    st = N.bn_stats(y2, EPS)
    e_mean, e_rstd = N.bn_stat_bounds(y2, st, *stats_n_p(route_f), EPS)
    ref = tail_reference(ti, st, e_mean, e_rstd)
    yd = _dev_rows(G_, y2, C, dt)
    st_dev = torch.full((C, 2), math.nan, device=G_.DEV); scratch = _out_rows(G_, rows, C, C, dt)
    gad, bed = ti["ga"].float().to(G_.DEV), ti["be"].float().to(G_.DEV)
    G_.check(G_.lib.eegldm_batchnorm_lrelu_fwd(c.h, G_.ptr(yd), C, G_.ptr(gad), G_.ptr(bed), G_.ptr(st_dev), None, None, None, G_.ptr(scratch), C, rows, C, SLOPE, 1, dt))
    torch.cuda.synchronize()
    _confirm(G_, 0, route_f, tag)
    fails += tail_judge(tail_run(G_, c, ti, dt, tag, st_dev=st_dev), ti, ref, tag)
    # refusals: an ineligible channel count and a leading dimension that is no multiple of the 16-byte chunk
    E = 4 if dt == 0 else 8
    buf = torch.zeros(B * L * 128, device=G_.DEV); lg = torch.zeros(B * L, device=G_.DEV)
    for Cb, ldb in ((24, 24), (C, C + E // 2)):
        rc = G_.lib.eegldm_debug_disc_tail_fwd(c.h, dt, G_.ptr(buf), ldb, G_.ptr(buf), G_.ptr(buf), G_.ptr(buf), G_.ptr(buf), None, SLOPE, G_.ptr(lg), B, L, Cb)
        assert rc == -3, f"tail C{Cb} ld {ldb} [{FMT[dt]}]: return code {rc}, expected EEGLDM_ERR_UNSUPPORTED"
        rc = G_.lib.eegldm_debug_disc_tail_bwd(c.h, dt, G_.ptr(buf), ldb, G_.ptr(buf), G_.ptr(buf), G_.ptr(buf), G_.ptr(buf), SLOPE, G_.ptr(lg), G_.ptr(buf), ldb,
                                               None, None, None, None, B, L, Cb)
        assert rc == -3, f"tail backward C{Cb} ld {ldb} [{FMT[dt]}]: return code {rc}, expected EEGLDM_ERR_UNSUPPORTED"
    print(f"[route] tail [{FMT[dt]}]: C 24 and ld {C + E // 2} refused")
    _raise(fails)


# ---------------------------------------------------------------- fused head
def head_inputs(B, L, C0, stride, dt, bias=True, acc=True, seed=211):
    fmt = FMT[dt]
    Lo = L // stride
    x = N.to_storage(_randn((B, L), seed), fmt)
    w = N.to_storage(_randn((3, C0), seed + 1) / math.sqrt(3.0), fmt)
    b = N.rne(0.3 * _randn((C0,), seed + 2), "f32") if bias else None
    da = N.to_storage(_randn((B, Lo, C0), seed + 3), fmt)
    start = dict(dw=N.rne(_randn((3, C0), seed + 4), "f32") if acc else torch.zeros(3, C0).double(),
                 db=N.rne(_randn((C0,), seed + 5), "f32") if acc else torch.zeros(C0).double())
    return dict(x=x, w=w, bias=b, da=da, start=start, fmt=fmt, B=B, L=L, Lo=Lo, C0=C0, stride=stride)


def head_reference(hi):
    x, w, bias, da, s = hi["x"], hi["w"], hi["bias"], hi["da"], hi["stride"]
    B, Lo, C0 = da.shape; rows = B * Lo
    u = N.U32
    z, zmag = N.head_z(x, w, bias, s, Lo)
    d = N.gamma(3 + 4) * zmag + (u * bias.abs() if bias is not None else 0.0)
    Uset = z.abs() <= d
    share = float(Uset.double().mean())
    assert share <= U_CAP, f"mask-uncertain share {share:.3e} above {U_CAP}: the case needs other inputs"
    m = z > 0
    dym = torch.where(m | Uset, da.abs(), SLOPE * da.abs())
    wid = torch.where(Uset, (1 - SLOPE) * da.abs(), torch.zeros_like(da))
    dw, db, dx = N.head_bwd(da, x, w, bias, SLOPE, s)
    ones = torch.ones_like(m)
    dw_m, db_m, dx_m = N.head_bwd(dym, x.abs(), w.abs(), None, 1.0, s, mask=ones)
    dw_w, db_w, dx_w = N.head_bwd(wid, x.abs(), w.abs(), None, 1.0, s, mask=ones)
    s0 = hi["start"]
    return dict(share=share, dw=dw + s0["dw"], db=db + s0["db"], dx=dx,
                b_dw=N.gamma(rows + 2) * (dw_m + s0["dw"].abs()) + dw_w, b_db=N.gamma(rows + 1) * (db_m + s0["db"].abs()) + db_w,
                b_dx=N.gamma(3 * C0 + 2) * dx_m + dx_w)


def head_judge(got, hi, ref, tag):
    fails = []
    print(f"[numerics] {tag} mask-uncertain share {ref['share']:.2e} (cap {U_CAP})")
    for k in ("dw", "db", "dx"):
        if k in got:
            try:
                N.check_abs(got[k], ref[k], ref["b_" + k], "f32", route=f"{tag} {k}")
            except AssertionError as e:
                fails.append((k, str(e)))
    return fails


def head_run(G_, c, hi, dt, tag, want=("dw", "dx")):
    B, L, Lo, C0, s = hi["B"], hi["L"], hi["Lo"], hi["C0"], hi["stride"]
    f32 = lambda t: t.float().to(G_.DEV).contiguous()
    dad = hi["da"].reshape(B * Lo, C0).to(G_.TDT[dt]).to(G_.DEV).contiguous()
    xd = hi["x"].to(G_.TDT[dt]).to(G_.DEV).contiguous(); wd = hi["w"].to(G_.TDT[dt]).to(G_.DEV).contiguous()
    bd = f32(hi["bias"]) if hi["bias"] is not None else None
    dw, db = f32(hi["start"]["dw"]), f32(hi["start"]["db"])
    dx = torch.full((B, L), math.nan, device=G_.DEV)
    G_.check(G_.lib.eegldm_debug_disc_head_bwd(c.h, dt, G_.ptr(dad), C0, G_.ptr(xd), G_.ptr(wd), G_.ptr(bd), SLOPE, G_.ptr(dw) if "dw" in want else None,
                                               G_.ptr(db) if "dw" in want else None, G_.ptr(dx) if "dx" in want else None, B, L, Lo, C0, s))
    torch.cuda.synchronize()
    G_n, NJ = tail_shape(C0, dt)
    print(f"[route] {tag}: head_bwd {' + '.join(('pg' if k == 'dw' else 'dx') for k in want)}<{FMT[dt]}, G={G_n}, NJ={NJ}> stride={s} L={L}")
    got = {}
    if "dw" in want:
        got.update(dw=dw.cpu().double(), db=db.cpu().double())
    else:
        assert torch.equal(dw.cpu().double(), hi["start"]["dw"]) and torch.equal(db.cpu().double(), hi["start"]["db"]), f"{tag}: dw / db changed although not asked for"
    if "dx" in want:
        got["dx"] = dx.cpu().double()
    else:
        assert bool(torch.isnan(dx).all()), f"{tag}: dx written although not asked for"
    return got


HEAD_GEOM = [(2, 5, 16), (2, 3, 74), (1, 3, 37)]      # stride, B, L: Lo = 8 < one step of the row walk (b++ and the clamped sample index); a long stride-2; stride 1


@pytest.mark.parametrize("geom", HEAD_GEOM, ids=[f"stride{s} B{b} L{l}" for s, b, l in HEAD_GEOM])
@pytest.mark.parametrize("dt", [0, 1, 2], ids=["f32", "bf16", "f16"])
def test_fused_head_every_instantiation(dt, geom, env_switches):
    G_ = _G(); c = G_.ctx()
    s, B, L = geom
    fails = []
    for i, C0 in enumerate(TAIL_C[dt]):
        bias = i % 2 == 0
        tag = f"head C{C0} stride {s} B{B} L{L}{'' if bias else ' no bias'} [{FMT[dt]}]"
        hi = head_inputs(B, L, C0, s, dt, bias=bias, acc=True)
        ref = head_reference(hi)
        fails += head_judge(head_run(G_, c, hi, dt, tag), hi, ref, tag)
        if C0 == 64:
            fails += head_judge(head_run(G_, c, hi, dt, tag + " dx alone", want=("dx",)), hi, ref, tag + " dx alone")
            fails += head_judge(head_run(G_, c, hi, dt, tag + " dw alone", want=("dw",)), hi, ref, tag + " dw alone")
    if s == 2:      # an odd length is refused by the eligibility check
        buf = torch.zeros(4096, device=G_.DEV)
        rc = G_.lib.eegldm_debug_disc_head_bwd(c.h, dt, G_.ptr(buf), 64, G_.ptr(buf), G_.ptr(buf), None, SLOPE, G_.ptr(buf), None, None, 2, 15, 8, 64, 2)
        assert rc == -3, f"head stride 2 L 15 [{FMT[dt]}]: return code {rc}, expected EEGLDM_ERR_UNSUPPORTED"
        print(f"[route] head stride 2 L 15 [{FMT[dt]}]: refused")
    _raise(fails)


# ---------------------------------------------------------------- the shared sum areas, call after call
@pytest.mark.parametrize("modes", ["non-deterministic", "deterministic", "alternating"])
def test_sum_area_sequence(modes, env_switches):
    """BN bwd C 64 -> tail bwd C 512 (bf16) -> BN bwd C 12 -> head bwd C0 64 -> tail bwd C 32 -> BN bwd C 64 on one context and stream: the
    folds of widths 2 C, 5 C + 1 and 4 C0 alternate between the two sum areas, each re-zeroing the other for the next call.  A stale or
    un-zeroed area is off by whole sums, far outside any bound."""
    G_ = _G(); c = G_.ctx()
    bn64 = next(cs for cs in BN_CASES if cs[0] == "4-wide fold_finalize"); bn12 = next(cs for cs in BN_CASES if cs[0].startswith("4-wide C12"))
    steps = [("bn", bn64, 0), ("tail", 512, 1), ("bn", bn12, 0), ("head", 64, 1), ("tail", 32, 0), ("bn", bn64, 2)]
    fails = []
    for i, (kind, what, dt) in enumerate(steps):
        det = modes == "deterministic" or (modes == "alternating" and i % 2 == 1)
        env_switches(EEGLDM_DETERMINISTIC="1" if det else None)
        tag = f"sequence ({modes}) step {i + 1} {kind} {'det' if det else 'non-det'}"
        if kind == "bn":
            case = what[:7] + ("det" if det else "",)
            off = 30.0
            inp = bn_inputs(case, dt, off)
            ref = bn_reference(inp, expected_route(inp["rows"], inp["C"], True, det, "train", 0))
            fails += bn_judge(bn_run(G_, c, case, dt, inp, env_switches, tag), inp, ref, tag)
        elif kind == "tail":
            ti = tail_inputs(3, 37, what, dt, seed=300 + i)
            ref = tail_reference(ti)
            fails += tail_judge(tail_run(G_, c, ti, dt, tag, fwd=False), ti, ref, tag)
        else:
            hi = head_inputs(3, 74, what, 2, dt, seed=300 + i)
            ref = head_reference(hi)
            fails += head_judge(head_run(G_, c, hi, dt, tag, want=("dw",)), hi, ref, tag)
    _raise(fails)


# ---------------------------------------------------------------- column statistics of the weight-stationary convs
# name, (B, L, Cin, Cout, stride), pack, kernel that must serve it, statistics expected
ST_CASES = [
    ("conv_ws 128->256 M16512", (86, 192, 128, 256, 1), None, "conv_ws", True),
    ("conv_ws2 stride2 128->256 M8192", (64, 256, 128, 256, 2), None, "conv_ws2", True),
    ("conv_ws paired rows stride2 64->128 M16384", (128, 256, 64, 128, 2), "s2", "conv_ws", True),
    ("conv_ws M16320 (below the threshold)", (85, 192, 128, 256, 1), None, None, False),
    ("conv_ws2 M8064 (below the threshold)", (63, 256, 128, 256, 2), None, None, False),
    ("paired rows M16256 (below the threshold)", (127, 256, 64, 128, 2), "s2", None, False),
]


def _prof_rows(G_, c):
    path = os.path.join(tempfile.gettempdir(), f"eegldm_bn_rounding_rows_{os.getpid()}.csv")
    G_.check(G_.lib.eegldm_prof_dump(c.h, path.encode()))
    with open(path) as fh:
        return list(csv.DictReader(fh))


def _conv_colstats(G_, c, x, w, bias, dims, pack, dt):
    """run eegldm_debug_conv1d_fwd_colstats; returns (profiled kernel names, nparts, partials (nparts, 2 Cout) float64, y (rows, Cout) float64)"""
    B, L, Cin, Cout, s = dims
    Lout = L // s
    xd, wd = G_.nlc(x, dt), G_.pack_w(w, dt)
    bd = bias.float().to(G_.DEV) if bias is not None else None
    yd = torch.full((B * Lout, Cout), math.nan, device=G_.DEV, dtype=G_.TDT[dt])
    parts = torch.full((4 << 20,), math.nan, device=G_.DEV)                # the 16 MiB the library's own caller provides
    nparts = ctypes.c_int(-1)
    keep = []
    if pack == "s2":
        keep += [torch.empty(3 * 128 * 128, device=G_.DEV, dtype=G_.TDT[dt]) for _ in range(2)]
        G_.check(G_.lib.eegldm_conv1d_pack_stride2(c.h, G_.ptr(wd), G_.ptr(keep[0]), G_.ptr(keep[1]), Cout, Cin, dt))
    try:
        c.prof_enable(True)
        G_.check(G_.lib.eegldm_debug_conv1d_fwd_colstats(c.h, G_.ptr(xd), Cin, G_.ptr(wd), G_.ptr(bd), G_.ptr(yd), Cout, B, L, Cin, Cout, 3, s, 1, 1,
                                                         None, 0, None, 0, dt, G_.ptr(parts), ctypes.byref(nparts)))
        torch.cuda.synchronize()
        rows = _prof_rows(G_, c)
    finally:
        c.prof_enable(False)
        if pack:
            G_.check(G_.lib.eegldm_conv1d_forget_kblocked(c.h, G_.ptr(wd)))
    n = nparts.value
    assert n >= 0, "col_nparts was not written"
    assert bool(torch.isnan(parts[n * 2 * Cout:]).all()), "partials written past the rows reported"
    return [r["kernel"] for r in rows], n, parts[:n * 2 * Cout].reshape(n, 2 * Cout).double().cpu(), yd.double().cpu(), parts


@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", ST_CASES, ids=_ids(ST_CASES))
def test_conv_column_statistics(case, dt, env_switches):
    G_ = _G(); c = G_.ctx()
    name, dims, pack, kernel, has_stats = case
    B, L, Cin, Cout, s = dims
    fmt = FMT[dt]
    Lout = L // s; rows = B * Lout
    x = N.to_storage(_randn((B, Cin, L), 221), fmt)
    w = N.to_storage(_randn((Cout, Cin, 3), 222) / math.sqrt(3 * Cin), fmt)
    if not has_stats:
        kerns, n, _p, _y, _buf = _conv_colstats(G_, c, x, w, None, dims, pack, dt)
        print(f"[route] {name} [{fmt}]: served by {kerns}, col_nparts = {n}")
        assert n == 0 and not any(k.startswith("conv_ws") for k in kerns), f"{name}: col_nparts = {n}, kernels {kerns}"
        return
    to_rows = lambda t: t.permute(0, 2, 1).reshape(rows, Cout)
    y0 = to_rows(N.conv1d_fwd(x, w, None, s, 1, 1)); m0 = to_rows(N.conv1d_fwd(x.abs(), w.abs(), None, s, 1, 1))       # shared by both bias runs
    sigma = float(y0.std())
    fails = []
    for what, bias in (("bias 0", torch.zeros(Cout, dtype=torch.float64)), ("bias 30 sigma", N.rne(sigma * (30 + _randn((Cout,), 223)), "f32"))):
        tag = f"{name} {what} [{fmt}]"
        y, mag = y0 + bias, m0 + bias.abs()
        S1, S2 = N.col_stats(y)
        dy = N.gamma(3 * Cin + 4) * mag
        b1 = N.gamma(rows + 3 * Cin + 4) * mag.sum(0)
        b2 = (2 * y.abs() * dy + dy * dy).sum(0) + N.gamma(rows + 2) * S2
        kerns, n, parts, yd, buf = _conv_colstats(G_, c, x, w, bias, dims, pack, dt)
        assert kerns == [kernel], f"{tag}: served by {kerns}, expected {kernel}"
        assert n > 0, f"{tag}: the kernel left no column statistics"
        print(f"[route] {tag}: {kerns[0]} with column statistics, {n} partial rows x {2 * Cout}")
        got = parts.sum(0).reshape(Cout, 2)
        for k, ref_, bnd in ((0, S1, b1), (1, S2, b2)):
            try:
                N.check_abs(got[:, k], ref_, bnd, "f32", route=f"{tag} column {'sum' if k == 0 else 'sum of squares'}")
            except AssertionError as e:
                fails.append((f"S{k + 1}", str(e)))
        # the fold the discriminator runs on these partials
        pi = dict(parts=parts, n=rows, C=Cout, nparts=n, rm=torch.zeros(Cout, dtype=torch.float64), rv=torch.ones(Cout, dtype=torch.float64), nbt=0.0)
        pref = parts_reference(pi)
        st = torch.full((Cout, 2), math.nan, device=G_.DEV)
        rm, rv, nbt = torch.zeros(Cout, device=G_.DEV), torch.ones(Cout, device=G_.DEV), torch.zeros(1, device=G_.DEV)
        G_.check(G_.lib.eegldm_debug_bn_stats_from_parts(c.h, G_.ptr(buf), n, G_.ptr(st), G_.ptr(rm), G_.ptr(rv), G_.ptr(nbt), rows, Cout))
        torch.cuda.synchronize()
        _confirm(G_, 0, dict(stats=PARTS, blocks=n), tag)
        std = st.cpu().double()
        fails += parts_judge(dict(st=std, rm=rm.cpu().double(), rv=rv.cpu().double(), nbt=float(nbt)), pi, pref, tag + " fold")
        # reported, not asserted: these statistics (of the unrounded outputs) against float64 and against those of the rounded y that the apply pass reads
        t64 = N.bn_stats(y, EPS); tr = N.bn_stats(yd, EPS)
        print(f"[numerics] {tag} statistics of the unrounded outputs: rstd within {float((std[:, 1] / t64['rstd'] - 1).abs().max()):.2e} of float64, "
              f"{float((std[:, 1] / tr['rstd'] - 1).abs().max()):.2e} of the rounded y's; mean within {float(((std[:, 0] - tr['mean']).abs() * tr['rstd']).max()):.2e} sigma of the rounded y's; "
              f"mean^2 / var up to {float((t64['mean'] ** 2 / t64['var']).max()):.3g}")
    _raise(fails)
