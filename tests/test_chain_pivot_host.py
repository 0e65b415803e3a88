"""The inputs of test_chain_pivot_gpu.py, checked on the CPU: for every case the census (chain_pivot_ref.census, the kernels'
elimination order and threshold rule in float64) solves the system, the system and every block that is inverted are well
conditioned, no pivot decision is within 1e-6 of the threshold -- so rounding in the device's order of summation cannot flip
one and the census says what the device swaps -- and rows ARE swapped where the GPU test is meant to exercise the swap code.  No
GPU case can pass because its input happened not to swap."""
import os
import re

import numpy as np
import pytest

import chain_pivot_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"T{T}-n{n}-{gen}" for T, n, gen in R.CASES]


def test_plan_restatement_matches_chain_plan_hpp():
    """chain_passes restates chain_plan.hpp::chain_passes; the library exposes no call for the plan, so the two expressions that
    decide it are compared with the header's text, and the restatement with the issue's table of (cap, S)."""
    src = open(os.path.join(ROOT, "gaussianvi_amd", "csrc", "chain_plan.hpp")).read()
    assert re.search(r"const int m_seg = " + re.escape(R.MSEG_EXPR) + ";", src)
    assert re.search(r"const int cap = " + re.escape(R.CAP_EXPR) + ";", src)
    assert re.search(r"for \(int N : \{" + ", ".join(map(str, R.PADDED)) + r"\}\)", src)
    for N, cap, S in ((2, 128, 32), (3, 64, 32), (4, 64, 32), (6, 48, 32), (8, 24, 16), (12, 8, 8), (16, 8, 8)):
        assert len(R.chain_passes(cap, N)) == 1 and R.chain_passes(cap + 1, N)[0] == (0, S.bit_length() - 1, False)
    assert [len(R.chain_passes(T, 2)) for T in (65, 66, 128, 129, 4096, 4097)] == [1, 1, 1, 2, 2, 3]
    assert [len(R.chain_passes(T, 12)) for T in (8, 9, 64, 65)] == [1, 2, 2, 3]
    assert R.chain_passes(1537, 6) == [(0, 5, False), (5, 5, False), (10, 1, True)]


def test_case_table_is_the_issues():
    assert len(R.CASES) == 2 + 8 + 14 + 12 + 12 + 21 + 10 + 3 * 12
    assert all(R.padded(n) == N for n, N in ((1, 1), (2, 2), (3, 3), (4, 4), (5, 6), (6, 6), (7, 8), (8, 8), (9, 12), (11, 12),
                                             (12, 12), (13, 16), (16, 16)))
    zero = sorted((n, T) for T, n, gen in R.CASES if gen == "zero")
    assert [T for n, T in zero if n == 2] == [2, 3, 129] and [T for n, T in zero if n == 6] == [3, 35, 49]
    assert [T for n, T in zero if n == 8] == [2, 3, 25] and [T for n, T in zero if n == 16] == [3, 8, 9]


@pytest.mark.parametrize("T,n,gen", R.CASES, ids=IDS)
def test_case_is_well_posed_and_swaps_where_it_must(T, n, gen):
    D, U, rhs, x, info = R.case(T, n, gen)
    assert np.array_equal(D, np.swapaxes(D, 1, 2))
    assert min(np.linalg.eigvalsh(Dt).min() for Dt in D) < 0.0       # a diagonal block is not positive definite: nor is the chain
    assert [r["level"] for r in info] == [R.node_level(e, T) for e in range(T)]
    if T * n <= 1600:
        A = R.dense(D, U)
        ref = np.linalg.solve(A, rhs.reshape(-1))
        err = np.abs(x.reshape(-1) - ref).max() / np.abs(ref).max()
        cond = np.linalg.cond(A)
        print(f"census against the dense solve {err:.2e}, cond {cond:.2f}")
        assert err < 1e-12
        assert cond <= 1e2
    res = R.block_residual(D, U, x, rhs)
    assert res < 1e-12 * max(1.0, np.abs(D).max()) * max(1.0, np.abs(x).max())
    nsw = sum(bool(r["swaps"]) for r in info)
    print(f"{nsw} of {T} nodes swap; worst block cond {max(r['cond'] for r in info):.2f}, closest decision "
          f"{min(r['margin'] for r in info):.2e}")
    assert R.case_problems(T, n, info) == []
    if gen == "zero":
        exact, high = R.zero_nodes(T)
        assert all(D[e, 0, 0] == 0.0 and info[e]["level"] == 0 for e in exact)
        assert all(info[e]["swaps"] and info[e]["swaps"][0][0] == 0 for e in exact + high)
        assert 0 in high and any(e + 1 >= T for e in exact) == (T % 2 == 0)
        for e in high:                                               # effective leading entry at 1e-3 of its column maximum
            B = info[e]["block"]
            assert abs(B[0, 0] / np.abs(B[1:, 0]).max() - 1e-3) < 1e-9


@pytest.mark.parametrize("N", [2, 3, 4, 6, 8, 12, 16])
def test_swaps_of_a_block_size_cover_every_step_and_position(N):
    """Over the cases of one padded size together: a swap at the first step, at the last step that has a choice (p = n - 2), into
    the last row (rs = n - 1), two or more swaps in one node (n >= 3: a 2 x 2 block has one step with a choice), a swapped node
    without a right neighbour, a swapped root; and for the padded sizes at least that much for a block that IS padded."""
    for only_padded in (False, True):
        seen = set()
        for T, n, gen in R.CASES:
            if R.padded(n) != N or n < 2 or (only_padded and n == N):
                continue
            info = R.case(T, n, gen)[4]
            for e, r in enumerate(info):
                if not r["swaps"]:
                    continue
                seen |= {"p0"} if any(p == 0 for p, _ in r["swaps"]) else set()
                seen |= {"p_last"} if any(p == n - 2 for p, _ in r["swaps"]) else set()
                seen |= {"rs_last"} if any(rs == n - 1 for _, rs in r["swaps"]) else set()
                seen |= {"two"} if len(r["swaps"]) >= 2 else set()
                seen |= {"no_right"} if e > 0 and e + (1 << r["level"]) >= T else set()
                seen |= {"root"} if e == 0 else set()
        if only_padded and N <= 4:                       # (no n below these sizes is padded to them)
            continue
        want = {"p0", "p_last", "rs_last", "no_right", "root"} | ({"two"} if N >= 3 else set())
        assert seen >= want, (N, only_padded, sorted(want - seen))
