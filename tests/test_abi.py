"""CPU-only checks of the boundary: the C-ABI library builds/loads, exports every symbol declared in
include/gvi_hip.h, fails loudly without a GPU, and its HOST-side sparse-grid generator reproduces the
oracle / golden tables bit-exactly (sigma-point indices)."""
import os
import re

import numpy as np
import pytest

import gvi_oracle as o
from gaussianvi_amd import _lib, api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _declared():
    src = open(os.path.join(ROOT, "include", "gvi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gvi_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = _declared()
    assert len(names) >= 40
    bound = set(_lib.SIGNATURES) | set(_lib.STRING_GETTERS)
    for name in names:
        assert hasattr(lib, name), f"{name} declared in gvi_hip.h but not exported"
        assert name in bound, f"{name} has no ctypes signature"
    assert bound <= set(names)


def test_no_gpu_fails_loudly(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(api.GviError) as e:
        api.Context(0)
    assert e.value.status == 2 and "no CPU fallback" in str(e.value)


def test_fp32_reports_unsupported(lib):
    import ctypes as C
    h = C.c_void_p()
    assert lib.gvi_ctx_create(0, api.GVI_F32, C.byref(h)) == 3


@pytest.mark.parametrize("d,p", [(1, 10), (5, 2), (4, 3), (2, 10), (6, 5)])
def test_generator_matches_golden_tables_bit_exact(lib, golden_dir, d, p):
    g = np.load(os.path.join(golden_dir, "spgh_tables.npz"))
    Z, w, idx = api.spgh_nodes(d, p)
    assert np.array_equal(Z, g[f"Z_{d}_{p}"])                # bit-exact nodes
    assert np.array_equal(idx, g[f"idx_{d}_{p}"])            # bit-exact (level, node, sign) indices
    assert np.allclose(w, g[f"w_{d}_{p}"], rtol=1e-12, atol=1e-15)


def test_generator_12_5_headline_table(lib, golden_dir):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden import idx_checksum
    g = np.load(os.path.join(golden_dir, "spgh_tables.npz"))
    Z, w, idx = api.spgh_nodes(12, 5)
    assert Z.shape[0] == int(g["N_12_5"]) == api.spgh_count(12, 5) == 17217
    assert np.array_equal(Z[:8], g["Zhead_12_5"]) and np.array_equal(Z[-8:], g["Ztail_12_5"])
    assert idx_checksum(idx) == int(g["idxsum_12_5"])
    assert np.allclose(w[:8], g["whead_12_5"], rtol=1e-11) and np.allclose(w[-8:], g["wtail_12_5"], rtol=1e-11)
    assert np.isclose(np.abs(w).sum(), float(g["wabs_12_5"]), rtol=1e-12)
    assert (w < 0).sum() == int(g["wneg_12_5"])
    assert np.array_equal(np.abs(Z).sum(axis=0), g["Zcolabs_12_5"])
    # rows ascending lexicographic, no duplicates
    order = np.lexsort(Z.T[::-1])
    assert np.array_equal(order, np.arange(len(Z)))
    assert len(np.unique(Z, axis=0)) == len(Z)


@pytest.mark.parametrize("d,p", [(1, 1), (1, 25), (2, 7), (3, 4), (7, 3), (20, 2), (13, 3)])
def test_generator_matches_oracle_more_shapes(lib, d, p):
    Z, w, idx = api.spgh_nodes(d, p)
    Zo, wo, io = o.nwspgr(d, p, True)
    assert np.array_equal(Z, Zo) and np.array_equal(idx, io)
    assert np.allclose(w, wo, rtol=1e-11, atol=1e-16)
    assert abs(w.sum() - 1) < 1e-9


def test_generator_rejects_untabulated(lib):
    with pytest.raises(api.GviError) as e:
        api.spgh_count(3, 26)
    assert e.value.status == 4


@pytest.mark.parametrize("p,lo,hi", [(5, 1.5e5, 3e5), (6, 1.5e6, 2.5e6)])
def test_wide_table_weight_cancellation(lib, p, lo, hi):
    """sum |w_i| / |sum w_i| of the d = 24 tables (2.0e5 at p = 5, 1.9e6 at p = 6, 1.5e7 at p = 7 -- the
    (24,7) figure is measured in the GPU suite): the reason config 5 runs in fp64."""
    Z, w, idx = api.spgh_nodes(24, p)
    ratio = np.abs(w).sum() / abs(w.sum())
    assert lo < ratio < hi, ratio
    assert abs(w.sum() - 1.0) < 1e-9


def test_documented_option_names_are_the_implemented_ones():
    """include/gvi_hip.h lists the names gvi_set_option accepts; the list must be the names of the table the implementation looks
    a name up in (gaussianvi_amd/csrc/options.hpp; a name documented but not implemented, or the other way round, is a drifted header)."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gvi_hip.h")).read()
    m = re.search(r"Names:(.*?)\*/\s*gvi_status gvi_set_option", header, re.S)
    assert m, "option list not found in the header"
    documented = set(re.findall(r"[a-z][a-z0-9_]+", m.group(1).replace("*", " ")))
    src = open(os.path.join(root, "gaussianvi_amd", "csrc", "options.hpp")).read()
    body = src[src.index("constexpr OptionRow OPTION_ROWS[] = {"):]
    body = body[:body.index("};")]
    implemented = set(re.findall(r'^  opt_[a-z0-9_]+\("([a-z0-9_]+)"', body, re.M))
    hip = open(os.path.join(root, "gaussianvi_amd", "csrc", "api_inspect.inc")).read()     # the file that defines gvi_set_option
    assert "option_set(ctx->opt, name, value" in hip[hip.index("gvi_status gvi_set_option("):], "gvi_set_option looks the name up in the table"
    assert documented == implemented, (sorted(documented - implemented), sorted(implemented - documented))


def test_in_tree_build_refuses_defines(monkeypatch):
    """The in-tree library is always the product build: a define (a timing build) is refused before hipcc runs."""
    def no_hipcc(*args, **kwargs):
        raise AssertionError("hipcc ran")
    monkeypatch.setattr(build, "_hipcc", no_hipcc)
    monkeypatch.setattr(build.subprocess, "run", no_hipcc)
    for out in (None, build.LIB):
        with pytest.raises(ValueError, match="in-tree"):
            build.build_lib(force=True, out=out, defines=("GVI_FUSED_TIMING",))


def test_variant_build_passes_defines(monkeypatch, tmp_path):
    """A build into another path (tools/build_variant.py) gets its defines on the compiler line."""
    cmds = []
    def fake_run(cmd, **kwargs):
        cmds.append(cmd)
        open(cmd[cmd.index("-o") + 1], "wb").close()
        return build.subprocess.CompletedProcess(cmd, 0, "", "")
    monkeypatch.setattr(build, "_hipcc", lambda: "hipcc")
    monkeypatch.setattr(build.subprocess, "run", fake_run)
    out = str(tmp_path / "libgvi_hip_timing.so")
    assert build.build_lib(force=True, out=out, defines=("GVI_FUSED_TIMING",)) == out
    assert os.path.exists(out) and "-DGVI_FUSED_TIMING" in cmds[0]


def test_product_sources_have_no_experiment_builds():
    """No wrong-result timing experiment (GVI_EXP_*) is compiled into the product sources."""
    csrc = os.path.join(ROOT, "gaussianvi_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, name), errors="replace") as f:
            assert "GVI_EXP_" not in f.read(), name
