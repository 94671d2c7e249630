"""The dense reference of hank_fake_news / hank_fake_news_het (CPU only): at a stationary point everything the eight kernels of
csrc/hank_jacobian.h compute has a closed dense form on the operators tests/ss_diff_cases.py builds from the CPU oracle's dual
arithmetic (`operators`: BV, PV, Bx, Px, Lam, Sp; points pt = e n_a + a):

    Y_0 = Px, Y_j = PV BV^(j-1) Bx (G, n_hh)      the policy response j periods before a unit shock to each input
    iota_j = Sp Y_j                               what that response moves in the lottery of its period
    E^o_0 = f_o, E^o_{u+1} = Lam' E^o_u           output o's expectation vectors
    F[u, j, k, o] = E^o_u . iota_j[:, k]
    Dv[j, k, o] = (D df_o/da') . Y_j[:, k] + [j == 0] d_{o,k}

with f = (a', c, (1+r) c^-gamma, z c^-gamma), c = (1+r) a + w z + tr - a', and the same-period effect d_{o,k} = D . (df_o/dc
(a, z, 1)_k), plus D . c^-gamma for Value at k = 0 (its own factor 1 + r): `ss_diff_cases.output_partials`, the closed forms of
`ss_diff_cases.reference`. Nothing here comes from the device or from hank_amd's fake-news code; tests/test_fake_news_ref_host.py
pins it against the oracle's unit-tangent outputs through `household_jacobian`.

The module ends with the launch arithmetic of `fake_news()` (csrc/hank_hip.hip) restated in plain integers (`geometry`) and the
shapes tests/test_gpu_fake_news_dense.py runs with what each must reach (`SHAPES`); tests/test_geom_host.py holds the two and the
source together."""
import numpy as np

import ss_diff_cases as S


def dense_fake_news(c, P, n_het):
    """c: a `ss_diff_cases.case` dict -> F (P, P, n_hh, n_het), Dv (P, n_hh, n_het), the layout of HouseholdBlock.fake_news_het;
    [..., 0] is the reference of HouseholdBlock.fake_news"""
    op, D = c["ref"]["op"], np.asarray(c["D"], dtype=np.float64)
    G, n_hh = c["orc"].G, len(c["x"])
    assert 1 <= n_het <= c["n_het"] and P >= 1
    Y = np.empty((P, G, n_hh))
    Y[0] = op["Px"]
    dV = op["Bx"]
    for j in range(1, P):
        Y[j] = op["PV"] @ dV
        dV = op["BV"] @ dV
    iota = np.einsum("gh,jhk->jgk", op["Sp"], Y)
    fp, fc, dcdx, u = S.output_partials(c)
    E = np.empty((n_het, P, G))
    E[:, 0] = np.stack(c["ref"]["f"][:n_het])
    for t in range(P - 1):
        E[:, t + 1] = E[:, t] @ op["Lam"]                 # (Lam' E_u)' = E_u' Lam
    F = np.einsum("oug,jgk->ujko", E, iota)
    Dv = np.einsum("og,jgk->jko", D[None, :] * fp[:n_het], Y)
    d = np.einsum("og,gk->ko", D[None, :] * fc[:n_het], dcdx)
    if n_het > 2:
        d[0, 2] += D @ u
    Dv[0] += d
    return F, Dv


def constant_path(c, P):
    """the household inputs of the stationary primal, (n_hh, P)"""
    return np.tile(np.asarray(c["x"])[:, None], (1, P))


# ---- what fake_news() launches at a shape -----------------------------------------------------------------------------------------
FN_SLICES = 16                       # S of fake_news(): the K split of k_fn_gemm
TRANSPOSE_TILE, GEMM_TILE, GEMM_KSTEP, BLOCK = 32, 64, 16, 256


def _tiles(n, tile):
    """-> (tiles, entries in the last one)"""
    k = -(-n // tile)
    return k, n - (k - 1) * tile


def geometry(G, n_hh, n_out, P):
    """fake_news()'s launch arithmetic at a shape, in plain integers -> dict of
    NP = P n_hh (columns of dpT and iota), MP = n_out P (rows of E); kchunk = ceil(G / 16) rounded up to 16 and `slices`, the k of
    each of the 16 K slices (0: an empty one); transpose_t, gemm_n, gemm_m, gemm_m_dv, impulse_y, expect: (tiles or blocks, live
    entries in the last)"""
    NP, MP = P * n_hh, n_out * P
    per_slice = -(-G // FN_SLICES)
    kchunk = -(-per_slice // GEMM_KSTEP) * GEMM_KSTEP
    slices = tuple(max(0, min(G, (z + 1) * kchunk) - z * kchunk) for z in range(FN_SLICES))
    assert sum(slices) == G
    return dict(NP=NP, MP=MP, kchunk=kchunk, slices=slices, transpose_t=_tiles(P, TRANSPOSE_TILE), transpose_g=_tiles(G, TRANSPOSE_TILE),
                gemm_n=_tiles(NP, GEMM_TILE), gemm_m=_tiles(MP, GEMM_TILE), gemm_m_dv=_tiles(n_out, GEMM_TILE),
                impulse_y=_tiles(NP, BLOCK), expect=_tiles(G, BLOCK))


# economy -> (n_a, n_e, n_hh, outputs of the family): what `ss_diff_cases.case` builds (the GPU module asserts it on the case)
ECONOMIES = {"ks30x3": (30, 3, 2, 3), "ks50x2": (50, 2, 2, 3), "hank30x3": (30, 3, 3, 4), "clamp": (190, 2, 2, 3), "ks40x16": (40, 16, 2, 3),
             "ks40x5": (40, 5, 2, 3), "gamma0.5": (40, 3, 2, 3), "gamma3": (40, 3, 2, 3), "ks64x4": (64, 4, 2, 3)}
# (economy, P) -> what the shape must reach, as entries of `geometry` at the family's full count of outputs
_KS30_SLICES = (16,) * 5 + (10,) + (0,) * 10           # K slices 0-5 live, slice 5 with 10 of 16 k, slices 6-15 empty
SHAPES = {
    # P below one transpose tile; one partial M tile and one partial N tile
    ("ks30x3", 2): dict(slices=_KS30_SLICES, transpose_t=(1, 2), gemm_n=(1, 4), gemm_m=(1, 6)),
    ("ks30x3", 7): dict(slices=_KS30_SLICES, transpose_t=(1, 7), gemm_n=(1, 14), gemm_m=(1, 21)),
    # the transpose tile exactly full in t, then one row over; NP = 64 (an exact N tile) and 66; the last live K slice holds 4 k
    ("ks50x2", 32): dict(slices=(16,) * 6 + (4,) + (0,) * 9, transpose_t=(1, 32), NP=64, gemm_n=(1, 64)),
    ("ks50x2", 33): dict(slices=(16,) * 6 + (4,) + (0,) * 9, transpose_t=(2, 1), NP=66, gemm_n=(2, 2)),
    # three inputs, four outputs; at P = 100 the second y block of k_fn_impulse has 44 live lanes, seven M tiles, the last partial
    ("hank30x3", 33): dict(NP=99, MP=132, gemm_m=(3, 4), gemm_m_dv=(1, 4), transpose_t=(2, 1)),
    ("hank30x3", 100): dict(NP=300, impulse_y=(2, 44), MP=400, gemm_m=(7, 16), gemm_m_dv=(1, 4)),
    # two live lanes in the second impulse block; five transpose tile rows, the last with one row
    ("ks30x3", 129): dict(NP=258, impulse_y=(2, 2), transpose_t=(5, 1)),
    # kchunk 32: the last live slice holds one full 16-chunk plus 12
    ("clamp", 12): dict(kchunk=32, slices=(32,) * 11 + (28,) + (0,) * 4, expect=(2, 124)),
    # mid[16] full; kchunk 48: 13 full slices, one of 16, two empty
    ("ks40x16", 12): dict(kchunk=48, slices=(48,) * 13 + (16,) + (0,) * 2, expect=(3, 128)),
    ("ks40x5", 12): dict(kchunk=16, expect=(1, 200)),
    ("gamma0.5", 12): dict(kchunk=16),
    ("gamma3", 12): dict(kchunk=16),
    # G = 256: k_fn_expect with exactly one full block, every K slice exactly one 16-chunk with no tail, NP = 32
    ("ks64x4", 16): dict(expect=(1, 256), kchunk=16, slices=(16,) * 16, NP=32),
}


def check_shape(name, P, G=None, n_hh=None, n_out=None):
    """assert what SHAPES claims for (name, P) on `geometry`; G, n_hh, n_out: those of a live case, which must be ECONOMIES'"""
    n_a, n_e, hh, outs = ECONOMIES[name]
    assert (G is None or G == n_a * n_e) and (n_hh is None or n_hh == hh) and (n_out is None or n_out == outs), (name, G, n_hh, n_out)
    g = geometry(n_a * n_e, hh, outs, P)
    for key, want in SHAPES[name, P].items():
        assert g[key] == want, (name, P, key, g[key], want)
    return g
