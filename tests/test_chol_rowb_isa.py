"""The row-broadcast form of the register Cholesky (kernels_prep.hpp, prep_chol_body<DT, ROWB>) is in the built gfx950 code
object where it belongs (CPU only: disassembles the in-tree library the way test_handover_isa.py does).

A factorisation of dimension d has d (d - 1) / 2 trailing updates and its inverse as many: each is one v_fmac_f64_dpp with a
row_newbcast control in the row-broadcast form, and each pivot is one v_mov_b64_dpp.
  * factor_fused_kernel<6,4,4,12,6> and <6,6,2,12,6> hold the d = 12 and d = 6 bodies: >= 2 * (66 + 15) updates, >= 18 pivots;
    <2,4,4,4,2> the d = 4 and d = 2 bodies: >= 2 * (6 + 1) updates, >= 6 pivots;
  * prep_all_kernel<EPLP, true> holds the bodies of d = 2, 4, 6, 8, 12: >= 2 * (1 + 6 + 15 + 28 + 66) updates;
  * prep_all_kernel<EPLP, false> (option chol_rowb 0) is the v_readlane form: no DPP broadcast at all.
The wait states in front of every one of these DPP reads are checked, for the whole library, by test_chain_pair_isa.py."""
import pytest

import test_handover_isa as isa


def _dpp(k):
    out = {}
    for mn, op, _ in k.ins:
        if "row_newbcast" in op:
            out[mn] = out.get(mn, 0) + 1
    return out


def _matching(pattern):
    found = {name: k for name, k in isa.kernels().items() if pattern in name}
    assert found, pattern
    return found


def _updates(*dims):
    return 2 * sum(d * (d - 1) // 2 for d in dims)


@pytest.mark.parametrize("inst, dims", [("<6, 4, 4, 12, 6>", (12, 6)), ("<6, 6, 2, 12, 6>", (12, 6)), ("<2, 4, 4, 4, 2>", (4, 2))])
def test_the_fused_pass_holds_the_row_broadcast_form(inst, dims):
    found = _matching(f"gvi::factor_fused_kernel{inst}(")
    assert len(found) == 1, sorted(found)
    (name, k), = found.items()
    d = _dpp(k)
    print(f"{name.split('(')[0]}: row_newbcast operations {d}")
    assert d.get("v_fmac_f64_dpp", 0) >= _updates(*dims), d
    assert d.get("v_mov_b64_dpp", 0) >= sum(dims), d


def test_the_prep_launch_holds_both_forms_in_instances_of_their_own():
    rowb, readlane = _matching("gvi::prep_all_kernel<"), {}
    for name in sorted(rowb):
        if ", false>(" in name:
            readlane[name] = rowb.pop(name)
    assert len(rowb) == 3 and len(readlane) == 3, (sorted(rowb), sorted(readlane))
    for name, k in sorted(rowb.items()):
        d = _dpp(k)
        print(f"{name.split('(')[0]}: row_newbcast operations {d}")
        assert ", true>(" in name, name
        assert d.get("v_fmac_f64_dpp", 0) >= _updates(2, 4, 6, 8, 12), (name, d)
        assert d.get("v_mov_b64_dpp", 0) >= 2 + 4 + 6 + 8 + 12, (name, d)
    for name, k in sorted(readlane.items()):
        assert _dpp(k) == {}, (name, _dpp(k))
        assert sum(1 for mn, _, _ in k.ins if mn == "v_readlane_b32") >= 2 * _updates(2, 4, 6, 8, 12), name
