"""A small model of the chain stage's decisions (gaussianvi_amd/csrc/chain_plan.hpp), written from the description of the
kernels' LDS arrays and of the launch rules, for tests/test_chain_plan_host.py: the answer of tests/stubs/chain_plan_check.cpp
to a `plan` command as a list of launches, and as the line the program prints.  Plain Python, nothing is read from the header."""

LDS_LIMIT = 160 * 1024                                   # bytes of dynamic LDS a chain kernel may be given
PADDED = (1, 2, 3, 4, 6, 8, 12, 16)                      # compiled block sizes
WAVE_N, WAVE_T = 2, 65                                   # the lane-per-node kernel: blocks up to 2 x 2, chains up to 65 states


def padded(n):
    return next((N for N in PADDED if 1 <= n <= N), 0)


def levels(T):
    return max(T - 1, 0).bit_length()


def threads(N):
    return 1024 if N <= 8 else 512


def ceil_div(a, b):
    return -(-a // b)


def passes(T, N):
    """[dict] of the forward passes: segmented passes of S = 2^m nodes per workgroup while more nodes are alive than the top
    pass takes, then the top pass; lp_off counts one log-pivot entry per wave of every workgroup of the earlier passes"""
    m_seg = {1: 5, 2: 5, 3: 5, 4: 5, 6: 5, 8: 4, 12: 3, 16: 3}[N]
    cap = {1: 128, 2: 128, 3: 64, 4: 64, 6: 48, 8: 24, 12: 8, 16: 8}[N]
    out, level0, lp = [], 0, 0
    while ceil_div(T, 1 << level0) > cap:
        blocks = ceil_div(T, 1 << (level0 + m_seg))
        out.append(dict(level0=level0, m=m_seg, S=1 << m_seg, top=0, first=int(level0 == 0), par=len(out) & 1, lp_off=lp, blocks=blocks))
        lp += blocks * (threads(N) // 64)
        level0 += m_seg
    out.append(dict(level0=level0, m=levels(T) - level0, S=ceil_div(T, 1 << level0), top=1, first=int(level0 == 0), par=len(out) & 1,
                    lp_off=lp, blocks=1))
    return out


def fwd_doubles(has_e, has_y, top, N, S, two_row):
    nn = N * N
    w = 2 * (S + 1) * nn + 2 * S * nn                    # both accumulators of S + 1 nodes; couplings and their fill-in
    if top:
        w += 3 * S * nn + (S * nn if has_e else 0)       # the factors E, GA, GB stay in LDS (+ one array of the selected inverse)
    if has_y:
        w += 2 * (S + 1) * N + ((2 * S + 1) * N if top else 0)      # right-hand sides of both accumulators (+ v and x)
    w += N + N % 2 + 128                                 # a zero block (even length), the log-det reduction
    if two_row:
        w += 96 + 128 + 2 * nn                           # log-pivot slots of the two-node levels; lane records, identity, zeros
    return w


def bwd_doubles(has_e, N, S):
    nn = N * N
    return (5 * (S + 1) * nn + 3 * S * nn if has_e else (S + 1) * N + S * N + 2 * S * nn) + 2


def asm_dense_shape(sets, n):
    """sets: [(K, d, nsp, data)]"""
    if not 1 <= len(sets) <= 2 or any(nsp != 0 or K < 1 or not data or d not in (n, 2 * n) for K, d, nsp, data in sets):
        return False
    return sum(d == 2 * n for _, d, _, _ in sets) <= 1 and sum(d == n for _, d, _, _ in sets) <= 1


def plan(T, n, on0=0, back0=0, on1=0, list=0, shape=0, wave=1, asm_dense=1, pair=1, merge=0):
    """(status, assemble, threads, npass, [launch]); launch = dict(kernel, form, nb0, nb, nbt, nb0c, lds, pass_, carried)"""
    assemble = "Off" if not list else "Dense" if asm_dense and shape and T > 1 else "Generic"
    N = padded(n)
    if not N:
        return "BlockSize", assemble, 0, 0, []
    back0 = on0 and back0
    if not on0 and not on1:
        return "Ok", assemble, 0, 0, []
    if wave and n <= WAVE_N and 1 <= T <= WAVE_T:
        return "Ok", assemble, 64, 0, [dict(kernel="Wave", form="Own", nb0=int(on0), nb=int(on0) + int(on1), nbt=0, nb0c=0, lds=0, pass_=None,
                                            carried=None)]
    ps = passes(T, N)
    thr = threads(N)

    def form(q):
        return "Own" if N != 6 else "TwoRow" if pair and q["S"] // 2 > thr // 128 else "Readlane"

    def fwd(q):
        two = form(q) == "TwoRow"
        return 8 * max(fwd_doubles(True, False, q["top"], N, q["S"], two) if on0 else 0, fwd_doubles(False, True, q["top"], N, q["S"], two) if on1 else 0)

    def bwd(q):
        return 8 * max(bwd_doubles(True, N, q["S"]) if back0 else 0, bwd_doubles(False, N, q["S"]) if on1 else 0)

    ops = int(on0) + int(on1)
    back = back0 or on1
    top = ps[-1]
    launches = [dict(kernel="Forward", form=form(q), nb0=q["blocks"] * int(on0), nb=q["blocks"] * ops, nbt=0, nb0c=0, lds=fwd(q), pass_=q, carried=None)
                for q in ps[:-1]]
    merged = merge and back and len(ps) >= 2 and max(fwd(top), bwd(ps[-2])) <= LDS_LIMIT
    if merged:
        c = ps[-2]
        nbc = c["blocks"] * (int(bool(back0)) + int(on1))
        launches.append(dict(kernel="TopBack", form=form(top), nb0=int(on0), nb=ops + nbc, nbt=ops, nb0c=c["blocks"] * int(bool(back0)),
                             lds=max(fwd(top), bwd(c)), pass_=top, carried=c))
    else:
        launches.append(dict(kernel="Forward", form=form(top), nb0=int(on0), nb=ops, nbt=0, nb0c=0, lds=fwd(top), pass_=top, carried=None))
    if back:
        for q in reversed(ps[:-2] if merged else ps[:-1]):
            launches.append(dict(kernel="Backward", form="Own", nb0=q["blocks"] * int(bool(back0)), nb=q["blocks"] * (int(bool(back0)) + int(on1)),
                                 nbt=0, nb0c=0, lds=bwd(q), pass_=q, carried=None))
    if any(l["lds"] > LDS_LIMIT for l in launches):
        return "Lds", assemble, thr, len(ps), []
    return "Ok", assemble, thr, len(ps), launches


PASS_KEYS = ("level0", "m", "S", "top", "first", "par", "lp_off", "blocks")


def line(p):
    """the program's answer to the plan command"""
    status, assemble, thr, npass, launches = p
    out = f"plan {status} {assemble} {thr} {npass}"
    for l in launches:
        out += f" | {l['kernel']} {l['form']} {l['nb0']} {l['nb']} {l['nbt']} {l['nb0c']} {l['lds']}"
        for q in (l["pass_"], l["carried"]):
            if q is not None:
                out += " : " + " ".join(str(q[k]) for k in PASS_KEYS)
    return out


def parse(text):
    """a line of the program back into (status, assemble, threads, npass, [launch])"""
    head, *rest = text.split(" | ")
    _, status, assemble, thr, npass = head.split()
    launches = []
    for item in rest:
        fields, *ps = item.split(" : ")
        kernel, form, *nums = fields.split()
        nb0, nb, nbt, nb0c, lds = map(int, nums)
        qs = [dict(zip(PASS_KEYS, map(int, q.split()))) for q in ps] + [None, None]
        launches.append(dict(kernel=kernel, form=form, nb0=nb0, nb=nb, nbt=nbt, nb0c=nb0c, lds=lds, pass_=qs[0], carried=qs[1]))
    return status, assemble, int(thr), int(npass), launches
