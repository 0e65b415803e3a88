"""The route rules of the factor stage (gaussianvi_amd/csrc/routes.hpp: decide_route), restated in Python: which kernel a set's
pass takes under a variant and how the pass is chunked, and the written-out instance lists.  tests/test_factor_routes_gpu.py
holds the device to it leg by leg, tests/test_routes_host.py holds the header to it on the CPU."""
import numpy as np

from gaussianvi_amd import api

QUAD, FIXED, RANGE, H2D, BODY, H3D, ARM, SEG2, SEG3 = (api.PSI_QUAD_PRIOR, api.PSI_FIXED_PRIOR, api.PSI_RANGE_1D, api.PSI_HINGE_SDF_2D,
                                                       api.PSI_HINGE_SDF_2D_BODY, api.PSI_HINGE_SDF_3D, api.PSI_HINGE_SDF_3D_ARM,
                                                       api.PSI_HINGE_SDF_2D_SEG, api.PSI_HINGE_SDF_3D_SEG)
REG = {RANGE: (1,), H2D: (2, 4, 6), BODY: (3, 6), H3D: (3, 6), SEG2: (4, 8, 12), SEG3: (6,), QUAD: (2, 4, 6, 8, 12),
       FIXED: (1, 2, 3, 4, 6, 8, 12)}                                  # with_reg_instance: 24
SREG = {QUAD: (4, 8, 12), FIXED: (6, 12)}                             # with_sreg_instance: 5
SCOST = {QUAD: (12,), FIXED: (6,)}                                    # with_scost_instance
SPLIT_D = (16, 20, 24)                                                # with_split_instance: m = d and m = d / 2 -> 6
ORBIT_M = (2, 6, 12, 14)                                              # with_orbit_instance (m = 2, 14: supports <= 4)
OPSI_ROWS = {RANGE: 1, H2D: 2, BODY: 3, H3D: 3, ARM: 7}               # with_orbit_psi_instance: 5, orbit_psi_rows
PREP = ((8, 1), (16, 4), (32, 16))                                    # with_prep_instance: (largest d, elements per lane)
CODE = dict(orbit=6, opsi=7, sreg=2, scost=2, reg=2, split=3, generic=1)   # gvi_profile_geometry


# ---- the rules, restated ----
def _ceil(a, b):
    return -(-a // b)


def _orbit_shape(Z):
    """(largest support, 64-lane tiles) of the table's sign-orbit form (orbits.hpp: classes by support size; supports of <= 3
    coordinates with several orbits each are stored support-major, split over f lanes where that costs less)"""
    walk = [0, 300, 800, 1300, 2500, 5200, 10800]
    supp = Z[(Z >= 0).all(axis=1)] != 0
    size = supp.sum(axis=1)
    tiles = 0
    for s in range(int(size.max()), 0, -1):
        cls = supp[size == s]
        slots = len(cls)
        if s <= 3 and slots:
            counts = np.unique(cls, axis=0, return_counts=True)[1]
            G = int(counts[0])
            if (counts == G).all() and G > 1:
                f = min((f for f in range(1, G + 1) if G % f == 0), key=lambda f: _ceil(len(counts) * f, 64) * (G // f * walk[s] + 600))
                slots = len(counts) * f
        tiles += _ceil(slots, 64)
    return int(size.max()), tiles


def _chunks(route, K, Z, nchunk_full=None):
    """(nchunk, chunk) of a pass on `route`; scost: the cost pass re-chunks the full pass's plan eight times finer"""
    N = len(Z)
    Np = _ceil(N, 256) * 256
    if route in ("orbit", "opsi"):
        tiles = _orbit_shape(Z)[1]
        return min(tiles, max(1, _ceil(4096, K)), max(1, tiles // 6)), Np
    if route == "split":
        tiles = Np // 64
        nch = min(max(1, _ceil(1024, K), _ceil(tiles, 16384)), tiles)
        chunk = _ceil(tiles, nch) * 64
        return _ceil(Np, chunk), chunk
    iters = Np // 256
    want = {"generic": _ceil(1024, K), "scost": 8 * (nchunk_full or 0)}.get(route, _ceil(2048, K))
    nch = min(max(1, want), max(1, iters))
    chunk = _ceil(iters, nch) * 256
    return _ceil(Np, chunk), chunk


def _route(kind, d, m, Z, variant, orbit_on=True, full=True):
    """plan_moments for a set with a generated table, no closed form, no caller's psi; None: refused (variant 2)"""
    v = 0 if variant == 7 else variant
    reg = d in REG.get(kind, ()) and (kind != QUAD or d == 2 * m) and v != 1
    if v == 2 and not reg:
        return None
    smax = _orbit_shape(Z)[0]
    if orbit_on and v in (0, 6) and kind in (QUAD, FIXED) and d <= 32 and (m in (6, 12) or (m in (2, 14) and smax <= 4)) and smax <= 6:
        return "orbit"
    if orbit_on and variant == 7 and kind in OPSI_ROWS and smax <= 4 and OPSI_ROWS[kind] <= d <= 32:
        return "opsi"
    if reg:
        if v in (0, 5) and not full and d in SCOST.get(kind, ()):
            return "scost"
        return "sreg" if v in (0, 5) and d in SREG.get(kind, ()) else "reg"
    if v != 1 and kind in (QUAD, FIXED) and d in SPLIT_D and m in (d, d // 2):
        return "split"
    return "generic"
