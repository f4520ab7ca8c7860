"""-m gpu: the ResBlock executor (csrc/net.hip res_forward / res_backward, through eegldm_block_forward / _backward) against the float64
reference of tests/resblock_reference.py, producer by producer.

res_backward decides per call which launch produces each bias gradient and the per-sample column sums behind the embedding gradient: the
weight-gradient GEMM's fused column sums, a staged vector added to one or both output-side biases, a direct column-sum kernel, the total of
the per-sample sums, and for the sums themselves the pipelined / full-slab / predicated resident GroupNorm backward, the column-sum
kernels or the FiLM backward.  Every case below names the producers it is there for and ASSERTS them from eegldm_debug_res_last_route
before any figure is judged; the per-sample sums are read through a one-hot embedding (resblock_reference.per_sample_sums).

Each case: eegldm_resblock_create, non-zero gradient contents bound (gradients must add onto them), forward, backward, read-out, route
assertion, then the checks; one [numerics] line per case (route, worst error over bound per check).  The lines of the first full run are
in profiles/resblock_numerics.txt.

Checks (resblock_reference.py; every magnitude comes from the float64 reference, none from an engine output):
  A  whole block against float64: y, dx, demb and every parameter gradient minus its preloaded contents.  16-bit engines: relative L2
     below gpu_util.bf16_gap_bound(gap), gap = the storage-emulating oracle's own distance from float64.  fp32 engine: the rule of
     assert_grad_bound (tests/test_gpu_usleep_train.py), 4 max(e32, r ||ref||), e32 = the float32 oracle's own distance from float64.
  B  out_layers.3.bias / skip_connection.bias against bias_grad(rne(dy)) and skip_connection.weight against conv1d_wgrad(xr, rne(dy)) by
     numerics.check's hard bound gamma(B Lout) * mag (xr = rne(x), or rne of its resampled copy in an up / down block).
  C  per-sample sums per (b, c): |ps - ref| <= 2 (2 u_s + gamma(L)) sum_l |dh1_ref| + A's bound of that tensor; between two producers on
     the same inputs |ps_A - ps_B| <= 2 (2 u_s + 2 gamma(L)) sum_l |dh1_ref|  (u_s = 2^-9 bf16, 2^-12 f16, 0 f32).
  D  in_layers.2.bias = emb_layers.1.bias (no use_scale_shift_norm): within 2 gamma(B) sum_b |ps| when the read-out says "total of the
     per-sample sums", else 2 (2 u_s + gamma(B L)) sum |dh1_ref|; out_layers.3.bias = skip_connection.bias within the two bounds of B.
  E  a NaN at dy[b0, c0, l0]: the NaN masks of dx, demb and the four bias gradients equal the float64 reference's; other samples' dx and
     demb rows stay finite.

Cases (B, cin, cout, L, updown, ssn; 32 groups) -- the smallest shapes that take the route:
  golden            2  32  32  32        f32        c2 bias by a direct column sum (the golden tests' shape)
  staged            3  64 128  96        f32        the staged vector feeds out_layers.3.bias AND skip_connection.bias
  staged split      = staged, EEGLDM_GN_NO_RESIDENT=1: split GN backward; ONE column-sum launch writes per-sample sums and total
  pipe              8 256 256  96        bf16 f16   EEGLDM_GN_PIPE_MIN_SLABS=1: GN2 pipelined, chunk 256; sums from GN; c1 bias from the GEMM
                                                    (cout = 256 is not < 256)
  pipe two slabs   16 128 128 192        bf16       + EEGLDM_GN_PIPE_MAX_SLOT=1: two slabs per workgroup; c1 bias = total of the sums
  full slab         = pipe, EEGLDM_GN_NO_PIPE=1: resident full-slab body (6 rows x 16 row lanes = 96) with column sums
  predicated        = pipe, EEGLDM_GN_NO_PIPE=1 EEGLDM_GN_NO_STREAM=1: the predicated resident body
  split             = pipe, EEGLDM_GN_NO_RESIDENT=1: split GN; column-sum kernel over the stored dh1
  own gemm          8 128 256  96        bf16 f16   c2 bias and skip bias each from their own weight-gradient GEMM
  no fused bias     = own gemm, EEGLDM_NO_FUSED_BIAS_GRAD=1: 16-bit column-sum kernel + staged vector
  deterministic     = pipe and own gemm, EEGLDM_DETERMINISTIC=1: no fused bias, ordered column sums, two runs bit-equal in every output
  film              8 128 128 192 ssn    f32 bf16   the FiLM backward produces the [scale | shift] rows
  down / up / down skip   8 64 64 64 down, 8 64 64 32 up, 8 64 128 64 down      f32 bf16
  odd groups        3  96 160  40        f32 bf16   3 and 5 channels per group: split GN with scalar loads on both norms; K = 120 is no
                                                    whole number of GEMM stages.  (The issue's table names scalar column sums here; with 32
                                                    groups every channel count is a multiple of 4 and the column-sum kernel is always its
                                                    4-wide form, so no shape of this block reaches the scalar one.)"""
import ctypes as C
import math

import pytest
import torch

import resblock_reference as R

pytestmark = pytest.mark.gpu

SPLIT, RESIDENT, PIPE = 1, 2, 3                      # GroupNorm backward families (eegldm_debug_gn_last_route)
FULL_SLAB, PREDICATED = 1, 2                         # resident bodies
PS_GN, PS_COLSUM, PS_FILM = 1, 2, 3                  # who wrote the per-sample sums
FIELDS = ("fwd", "gn2_family", "gn2_cc", "gn2_body", "gn1_family", "gn1_cc", "gn1_body", "ps", "b_c2", "b_sk", "b_c1", "det")
PIPE_ENV = dict(EEGLDM_GN_PIPE_MIN_SLABS="1")

SHAPES = {"golden": (2, 32, 32, 32, 0, 0), "staged": (3, 64, 128, 96, 0, 0), "pipe": (8, 256, 256, 96, 0, 0), "pipe2": (16, 128, 128, 192, 0, 0),
          "own gemm": (8, 128, 256, 96, 0, 0), "film": (8, 128, 128, 192, 0, 1), "down": (8, 64, 64, 64, 1, 0), "up": (8, 64, 64, 32, 2, 0),
          "down skip": (8, 64, 128, 64, 1, 0), "odd groups": (3, 96, 160, 40, 0, 0)}
# name: (shape, formats, switches, what the read-out must show)
CASES = {
    "golden": ("golden", ("f32",), {}, dict(fwd=1, b_c2=R.B_COLSUM, b_sk=R.B_NONE, b_c1=R.B_COLSUM)),
    "staged": ("staged", ("f32",), {}, dict(b_c2=R.B_STAGED, b_sk=R.B_STAGED)),
    "staged split": ("staged", ("f32",), dict(EEGLDM_GN_NO_RESIDENT="1"),
                     dict(gn2_family=SPLIT, gn1_family=SPLIT, ps=PS_COLSUM, b_c1=R.B_COLSUM, b_c2=R.B_STAGED, b_sk=R.B_STAGED)),
    "pipe": ("pipe", ("bf16", "f16"), PIPE_ENV, dict(gn2_family=PIPE, gn2_cc=256, ps=PS_GN, b_c1=R.B_GEMM, b_c2=R.B_GEMM, b_sk=R.B_NONE)),
    "pipe two slabs": ("pipe2", ("bf16",), dict(PIPE_ENV, EEGLDM_GN_PIPE_MAX_SLOT="1"), dict(gn2_family=PIPE, gn2_cc=128, ps=PS_GN, b_c1=R.B_TOTAL)),
    "full slab": ("pipe", ("bf16",), dict(EEGLDM_GN_NO_PIPE="1"), dict(gn2_family=RESIDENT, gn2_cc=256, gn2_body=FULL_SLAB, ps=PS_GN, b_c1=R.B_GEMM)),
    "predicated": ("pipe", ("bf16",), dict(EEGLDM_GN_NO_PIPE="1", EEGLDM_GN_NO_STREAM="1"),
                   dict(gn2_family=RESIDENT, gn2_cc=256, gn2_body=PREDICATED, ps=PS_GN, b_c1=R.B_GEMM)),
    "split": ("pipe", ("bf16",), dict(EEGLDM_GN_NO_RESIDENT="1"), dict(gn2_family=SPLIT, gn1_family=SPLIT, ps=PS_COLSUM, b_c1=R.B_GEMM)),
    "own gemm": ("own gemm", ("bf16", "f16"), {}, dict(b_c2=R.B_GEMM, b_sk=R.B_GEMM)),
    "no fused bias": ("own gemm", ("bf16",), dict(EEGLDM_NO_FUSED_BIAS_GRAD="1"), dict(b_c2=R.B_STAGED, b_sk=R.B_STAGED, det=0)),
    "film": ("film", ("f32", "bf16"), {}, dict(fwd=2, ps=PS_FILM)),
    "down": ("down", ("f32", "bf16"), {}, dict(fwd=1, b_sk=R.B_NONE)),
    "up": ("up", ("f32", "bf16"), {}, dict(fwd=1, b_sk=R.B_NONE)),
    "down skip": ("down skip", ("f32", "bf16"), {}, dict(fwd=1)),
    "odd groups": ("odd groups", ("f32", "bf16"), {}, dict(gn2_family=SPLIT, gn1_family=SPLIT, ps=PS_COLSUM)),
}
PARAMS = [(name, fmt) for name, (_s, fmts, _e, _x) in CASES.items() for fmt in fmts]
# every switch a case may set, cleared first so that a case runs on exactly its own
ALL_SWITCHES = ("EEGLDM_GN_NO_RESIDENT", "EEGLDM_GN_NO_PIPE", "EEGLDM_GN_NO_STREAM", "EEGLDM_GN_PIPE_MIN_SLABS", "EEGLDM_GN_PIPE_MAX_SLOT",
                "EEGLDM_NO_FUSED_BIAS_GRAD", "EEGLDM_DETERMINISTIC")


def _G():
    import gpu_util as G
    return G


_REF = {}


def _reference(shape_name, fmt):
    """(inputs, float64 reference, float32 oracle, storage-emulating oracle): computed once per shape and format, never modified"""
    if (shape_name, fmt) not in _REF:
        inp = R.make_inputs(*SHAPES[shape_name])
        o32, oq = R.yardsticks(inp, fmt)
        _REF[(shape_name, fmt)] = (inp, R.reference(inp, fmt), o32, oq)
    return _REF[(shape_name, fmt)]


def _route_text(rt):
    who = {0: "none", 1: "colsum", 2: "gemm", 3: "total", 4: "staged"}
    ps = {0: "none", 1: "gn", 2: "colsum", 3: "film"}
    return (f"fwd{rt['fwd']} gn2={rt['gn2_family']}/{rt['gn2_cc']}/{rt['gn2_body']} gn1={rt['gn1_family']}/{rt['gn1_cc']}/{rt['gn1_body']} ps={ps[rt['ps']]} "
            f"c2={who[rt['b_c2']]} sk={who[rt['b_sk']]} c1={who[rt['b_c1']]}" + (" det" if rt["det"] else ""))


def _engine(inp, fmt, dy=None):
    """one forward and backward of the block on the device: (got, route).  got: y, dx, demb, raw (gradient buffer contents), g (raw minus
    the preload, in fp32 as the yardsticks take it off)"""
    G = _G()
    dt = {"f32": G.F32, "bf16": G.BF16, "f16": G.F16}[fmt]
    B, L, Lo, ci, co = inp["B"], inp["L"], inp["Lo"], inp["cin"], inp["cout"]
    h = C.c_void_p()
    G.check(G.lib.eegldm_resblock_create(G.ctx().h, ci, co, R.EMB, R.GROUPS, inp["updown"], inp["ssn"], dt, C.byref(h)))
    try:
        n = int(G.lib.eegldm_block_num_params(h))
        name = C.create_string_buffer(256)
        off, numel, ndim, shape = C.c_long(), C.c_long(), C.c_int(), (C.c_int * 3)()
        entries = {}
        for i in range(G.lib.eegldm_block_num_entries(h)):
            G.check(G.lib.eegldm_block_entry(h, i, name, 256, C.byref(off), C.byref(numel), C.byref(ndim), shape))
            entries[name.value.decode()] = (off.value, numel.value, tuple(shape[k] for k in range(ndim.value)))
        assert set(entries) == set(inp["params"])
        flat, grad = torch.zeros(n), torch.zeros(n)
        for k, (o, m, shp) in entries.items():
            for buf, src in ((flat, inp["params"][k]), (grad, inp["preload"][k])):
                assert tuple(src.shape) == shp, (k, tuple(src.shape), shp)
                buf[o:o + m] = (src.permute(2, 0, 1) if len(shp) == 3 else src).reshape(-1)          # conv weights packed [K][Cout][Cin]
        flat, grad = flat.to(G.DEV), grad.to(G.DEV)
        G.check(G.lib.eegldm_block_bind(h, G.ptr(flat), G.ptr(grad)))
        x, emb = inp["x"].to(G.DEV), inp["emb"].to(G.DEV)
        dyd = (inp["dy"] if dy is None else dy).to(G.DEV)
        nan = lambda *s: torch.full(s, math.nan, device=G.DEV)               # an unwritten element shows
        y, dx, demb = nan(B, co, Lo), nan(B, ci, L), nan(B, R.EMB)
        G.check(G.lib.eegldm_block_forward(h, G.ptr(x), G.ptr(emb), G.ptr(y), B, L))
        G.check(G.lib.eegldm_block_backward(h, G.ptr(dyd), G.ptr(dx), G.ptr(demb)))
        torch.cuda.synchronize()
        out = (C.c_int * 12)()
        G.check(G.lib.eegldm_debug_res_last_route(out))
        route = dict(zip(FIELDS, out))
        gc = grad.cpu()
        raw = {}
        for k, (o, m, shp) in entries.items():
            t = gc[o:o + m]
            raw[k] = (t.reshape(shp[2], shp[0], shp[1]).permute(1, 2, 0) if len(shp) == 3 else t).reshape(shp).clone()
        g = {k: (raw[k] - inp["preload"][k].float()).double() for k in raw}
        return dict(y=y.cpu().double(), dx=dx.cpu().double(), demb=demb.cpu().double(), raw={k: v.double() for k, v in raw.items()}, g=g), route
    finally:
        G.lib.eegldm_block_destroy(h)


def _switch(env_switches, env):
    env_switches(**{k: env.get(k) for k in ALL_SWITCHES})


def _assert_route(tag, route, expect):
    bad = {k: (route[k], v) for k, v in expect.items() if route[k] != v}
    assert not bad, f"{tag}: the read-out shows {_route_text(route)}; (got, expected): {bad}"


@pytest.mark.parametrize("name,fmt", PARAMS, ids=[f"{n} {f}" for n, f in PARAMS])
def test_resblock_against_float64(name, fmt, env_switches):
    shape_name, _fmts, env, expect = CASES[name]
    inp, ref, o32, oq = _reference(shape_name, fmt)
    _switch(env_switches, env)
    got, route = _engine(inp, fmt)
    _assert_route(f"{name} {fmt}", route, expect)
    if name == "odd groups":      # GroupNorm 1 ran last: scalar loads (3 channels per group; GroupNorm 2's 5 fail the same vec4_ok test)
        gn1 = (C.c_int * 6)()
        _G().check(_G().lib.eegldm_debug_gn_last_route(1, gn1))
        assert tuple(gn1)[:2] == (SPLIT, 0), f"{name} {fmt}: GroupNorm 1 backward {tuple(gn1)}, expected the split family with scalar loads"
    rep = R.run_checks(got, ref, o32, oq, inp, fmt, route, collect=True)
    print(R.report_line(name, fmt, _route_text(route), rep))
    assert not rep["failed"], f"{name} {fmt} [{_route_text(route)}]: " + " | ".join(rep["failed"].values())


def test_per_sample_sum_producers_agree(env_switches):
    """C between producers: the pipelined, full-slab and predicated one-pass kernels and the column-sum kernel over the stored dh1, same inputs"""
    inp, ref, _o32, _oq = _reference("pipe", "bf16")
    ps = {}
    for name in ("pipe", "full slab", "predicated", "split"):
        _shape, _fmts, env, expect = CASES[name]
        _switch(env_switches, env)
        got, route = _engine(inp, "bf16")
        _assert_route(name, route, expect)
        ps[name] = R.per_sample_sums(got["g"]["emb_layers.1.weight"], inp["B"])
    names = list(ps)
    worst = {f"{a} / {b}": R.check_producers_agree(ps[a], ps[b], ref, "bf16") for i, a in enumerate(names) for b in names[i + 1:]}
    print("[numerics] resblock producers of the per-sample sums, |ps_A - ps_B| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("shape_name", ["pipe", "own gemm"])
def test_deterministic_mode(shape_name, env_switches):
    """EEGLDM_DETERMINISTIC=1: no bias gradient from a GEMM's fused (atomic) column sums, the ordered column-sum kernels, every check of
    the case, and two runs bit-equal in every output"""
    inp, ref, o32, oq = _reference(shape_name, "bf16")
    _switch(env_switches, dict(CASES[shape_name][2], EEGLDM_DETERMINISTIC="1"))
    (g1, route), (g2, route2) = _engine(inp, "bf16"), _engine(inp, "bf16")
    assert route == route2
    assert route["det"] == 1 and R.B_GEMM not in (route["b_c2"], route["b_sk"], route["b_c1"]), _route_text(route)
    if shape_name == "own gemm":
        _assert_route(shape_name, route, dict(b_c2=R.B_STAGED, b_sk=R.B_STAGED))
    rep = R.run_checks(g1, ref, o32, oq, inp, "bf16", route, collect=True)
    print(R.report_line("deterministic " + shape_name, "bf16", _route_text(route), rep))
    assert not rep["failed"], " | ".join(rep["failed"].values())
    bits = lambda t: t.float().contiguous().view(torch.int32)
    for k in ("y", "dx", "demb"):
        assert torch.equal(bits(g1[k]), bits(g2[k])), f"{k} differs between two deterministic runs"
    for k in g1["raw"]:
        assert torch.equal(bits(g1["raw"][k]), bits(g2["raw"][k])), f"gradient {k} differs between two deterministic runs"


@pytest.mark.parametrize("shape_name,fmt", [("staged", "f32"), ("staged", "bf16"), ("own gemm", "f32"), ("own gemm", "bf16")])
def test_nan_in_dy_stays_in_its_sample(shape_name, fmt, env_switches):
    """E"""
    inp, _ref, _o32, _oq = _reference(shape_name, fmt)
    _switch(env_switches, {})
    b0, c0, l0 = 1, 5, 7
    bad = dict(inp); bad["dy"] = inp["dy"].clone(); bad["dy"][b0, c0, l0] = math.nan
    ref = R.run_oracle(bad, fmt, torch.float64)
    assert bool(torch.isnan(ref["dx"][b0]).all()) and not bool(torch.isnan(ref["dx"][0]).any()) and bool(torch.isfinite(ref["demb"][0]).all())
    got, route = _engine(bad, fmt)
    R.check_nan_masks(got, ref)
    print(f"[numerics] resblock NaN in dy {shape_name:<10s} {fmt:>4s} route[{_route_text(route)}] masks of dx, demb and the bias gradients equal the reference's")
