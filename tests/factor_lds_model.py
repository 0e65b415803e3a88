"""An independent model of the factor stage's LDS layouts, written from the formulas the launches have always used (the issue
that introduced gaussianvi_amd/csrc/factor_lds.hpp lists them); it reads nothing from the header.  tests/test_factor_lds_host.py
compares the header's answers with it.  Offsets and sizes in doubles unless the name ends in _bytes; dd = d d, dp = d + (d & 1)."""

GEN_BS = 256
GENERIC_LIMIT = 160 * 1024
BOX_LIMIT = 64 * 1024


def npairs(d):
    return (d + 1) * (d + 2) // 2


def products(d):
    """A0 A1 V0 V1 [dd each] | al be [dp each] | lam [3d] | pa (int[dp]); Ll Xl [dd each] | Al [m d]; staging Sl [dd] | ml [d] one
    double behind; prep_kernel asks for (4dd + 2dp + 3d) 8 + dp 4 + 16 bytes, prep_all_kernel for
    (4dd + 2dp + 3d + (dp + 1) / 2 + 1 + dd + d) 8 + 16"""
    dd, dp = d * d, d + (d & 1)
    pa = 4 * dd + 2 * dp + 3 * d
    area = pa + (dp + 1) // 2
    return dict(A0=0, A1=dd, V0=2 * dd, V1=3 * dd, al=4 * dd, be=4 * dd + dp, lam=4 * dd + 2 * dp, pa=pa, jacobi_end=area,
                Ll=0, Xl=dd, Al=2 * dd, chol_end=3 * dd, doubles=area, Sl=area + 1, ml=area + 1 + dd, staged_end=area + 1 + dd + d,
                prep_bytes=(4 * dd + 2 * dp + 3 * d) * 8 + dp * 4 + 16,
                prep_all_bytes=(4 * dd + 2 * dp + 3 * d + (dp + 1) // 2 + 1 + dd + d) * 8 + 16)


def chol(d, m):
    return dict(chol_end=2 * d * d + m * d)


def epilogue(d):
    """Ms [npairs] | M2 Tm Sv Lv [dd each]; (npairs + 4dd) 8 bytes, epilogue_all_kernel 256 doubles more"""
    dd, n = d * d, npairs(d)
    return dict(Ms=0, M2=n, Tm=n + dd, Sv=n + 2 * dd, Lv=n + 3 * dd, end=n + 4 * dd, last=n + 4 * dd, doubles=n + 4 * dd, tree=n + 4 * dd,
                all_doubles=n + 4 * dd + 256)


def item(d):
    """the larger of (products area + staging + 2) and (epilogue area + 2), rounded to even"""
    dd, dp = d * d, d + (d & 1)
    prep = 4 * dd + 2 * dp + 3 * d + (dp + 1) // 2 + 1 + dd + d + 2
    epi = npairs(d) + 4 * dd + 2
    return dict(item=(max(prep, epi) + 1) & ~1, products=prep)


def helper(d, m):
    return dict(Al=0, mh=m * d, end=m * d + d)


# the walk's LDS per wave and what an item keeps outside the regions: the formulas of kernels_orbit.hpp / kernels_fused.hpp
def hstride(M):
    return 14 if M == 12 else M


def walk(d, M, copies):
    return (d * hstride(M) + copies * npairs(d) + 1) & ~1


def keep(dmax, M):
    return dmax * dmax + dmax * hstride(M) + M + (M & 1)


def fused(dmax, walk_doubles, keep_doubles, items):
    region = (max(walk_doubles, item(dmax)["item"]) + 1) & ~1
    return dict(region=region, lds=4 * region + items * (keep_doubles + 4 * npairs(dmax)))


def generic(d, m):
    """zs xs [256][d + 1] | cs [256] | Ssh [dd] | mush [d] | Ash [m d] | bsh gsh [m]; refused above 160 KB"""
    z = GEN_BS * (d + 1)
    o = dict(zs=0, xs=z, cs=2 * z, Ssh=2 * z + GEN_BS, mush=2 * z + GEN_BS + d * d, Ash=2 * z + GEN_BS + d * d + d)
    o["bsh"] = o["Ash"] + m * d
    o["gsh"] = o["bsh"] + m
    o["end"] = o["gsh"] + m
    o["bytes"] = (2 * GEN_BS * (d + 1) + GEN_BS + d * d + d + m * d + 2 * m) * 8
    o["refused"] = int(o["bytes"] > GENERIC_LIMIT)
    return o


def jko(d):
    return dict(M=0, Sg=d * d, Tm=2 * d * d, end=3 * d * d, bytes=3 * d * d * 8)


def fixed(d):
    return dict(box=d * d + 2 * d, box_refused=int((d * d + 2 * d) * 8 > BOX_LIMIT), halfspace=64 * d + 128,
                split=256 + 2 * d + 8 + 2 * 4 * 64 + 4 * 16 * 65 + 4 * 2 * 96, block3=item(8)["item"])


def line(values):
    return " ".join(f"{k}={v}" for k, v in values.items())


def parse(text):
    return {k: int(v) for k, v in (tok.split("=") for tok in text.split())}
