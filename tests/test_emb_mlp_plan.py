"""CPU: tile counts and the split-K partition of the time-embedding MLP kernels (csrc/emb_mlp_plan.h through eegldm_debug_emb_mlp_plan;
no device is touched)."""
import ctypes

import pytest

TILE, KC, MAX_SPLIT, SMALL_GRID = 64, 64, 32, 128


def plan(n, mc, te, E):
    from eegldm._lib import lib, check
    out = (ctypes.c_int * 12)()
    check(lib.eegldm_debug_emb_mlp_plan(n, mc, te, E, out))
    v = list(out)
    return dict(fwd=v[0:3], wgrad=v[3:6], dsemb_tiles=v[6], splits=v[7], kper=v[8], dh1_tiles=v[9], work=v[10] + (v[11] << 31))


def ceil(a, b):
    return -(-a // b)


def tiles(M, N, t):
    return ceil(M, t) * ceil(N, t)


def pick(tiles64):
    """32 x 32 tiles where 64 x 64 ones would make fewer than SMALL_GRID workgroups"""
    return 32 if tiles64 < SMALL_GRID else 64


def picked(M, N):
    return tiles(M, N, pick(tiles(M, N, TILE)))


def test_config_ldm_plan():
    p = plan(256, 128, 512, 6656)
    assert p["fwd"] == [128, 128, 416]          # 32 x 32 tiles: 8 x 16 (64 x 64 would be 32 workgroups); 64 x 64: 4 x 104
    assert p["wgrad"] == [832, 256, 64]         # E x te on 64 x 64; te x te and te x mc share a launch: 80 tiles of 64 -> 32 x 32
    assert p["dsemb_tiles"] == 32 and p["dh1_tiles"] == 128
    assert p["splits"] * p["dsemb_tiles"] >= 256      # the long reduction fills the chip
    assert p["work"] == (p["splits"] + 2) * 256 * 512


@pytest.mark.parametrize("n", [1, 3, 17, 63, 64, 65, 256, 1000])
@pytest.mark.parametrize("mc,E", [(32, 416), (32, 832), (128, 6656), (128, 13312), (4, 4), (36, 100)])
def test_split_partition_covers_the_reduction_exactly(n, mc, E):
    te = 4 * mc
    p = plan(n, mc, te, E)
    assert p["fwd"] == [picked(n, te), picked(n, te), picked(n, E)]
    tp = pick(tiles(te, te, TILE) + tiles(te, mc, TILE))
    assert p["wgrad"] == [picked(E, te), tiles(te, te, tp), tiles(te, mc, tp)]
    assert p["dsemb_tiles"] == tiles(n, te, TILE) and p["dh1_tiles"] == picked(n, te)
    s, kper = p["splits"], p["kper"]
    assert 1 <= s <= MAX_SPLIT and kper % KC == 0 and kper > 0
    # split z owns [z kper, min(E, (z + 1) kper)): every split non-empty, the last one reaches E
    assert (s - 1) * kper < E <= s * kper
    covered = sum(min(E, (z + 1) * kper) - z * kper for z in range(s))
    assert covered == E
    assert p["work"] == (s + 2) * n * te


def test_plan_refuses_empty_shapes():
    from eegldm._lib import lib
    out = (ctypes.c_int * 12)()
    assert lib.eegldm_debug_emb_mlp_plan(0, 32, 128, 416, out) != 0
    assert lib.eegldm_debug_emb_mlp_plan(4, 32, 128, 416, None) != 0
