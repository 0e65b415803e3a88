"""Where the host code of the library lives (gaussianvi_amd/csrc, DESIGN.md "Where the host code lives"): gvi_hip.hip is the index
of the one translation unit and defines nothing; the host code is in .inc fragments that it alone includes, in a fixed order; the
timing dump of the measurement build hangs off launch_factor.inc; no fragment outgrows what one reads in a sitting.  CPU only:
the sources are read, nothing is compiled."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianvi_amd", "csrc")
FRAGMENTS = ["host_ctx.inc", "launch_factor.inc", "launch_chain.inc", "api_setup.inc", "api_operators.inc", "ngd_stage.inc",
             "ngd_dist.inc", "ngd_iter.inc", "ngd_run.inc", "prox.inc", "dist_transport.inc", "api_inspect.inc", "posterior_host.inc"]
DATA = "gqn_table.inc"              # the tabulated rules of spgh.cpp: data, not host code of this unit
TIMING = "fused_timing.inc"         # under GVI_FUSED_TIMING only
MAX_LINES = 700


def _read(name):
    return open(os.path.join(CSRC, name), errors="replace").read()


def _code(text):
    """the text without comments (no string of these files holds a comment opener)"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _includers(target):
    pat = re.compile(r'^\s*#\s*include\s*"' + re.escape(target) + '"', re.M)
    return [name for name in sorted(os.listdir(CSRC)) if pat.search(_code(_read(name)))]


def test_the_unit_is_an_index():
    lines = [ln.strip() for ln in _code(_read("gvi_hip.hip")).splitlines() if ln.strip()]
    rest = [ln for ln in lines if not re.fullmatch(r'#include\s*(<[^>]+>|"[^"]+")', ln)]
    assert rest == ["using namespace gvi;", 'extern "C" {', "}"], rest
    # the bracket holds the entry-point fragments and nothing else of the host code sits before `using namespace gvi;`
    assert lines.index("using namespace gvi;") < lines.index('#include "host_ctx.inc"') < lines.index('extern "C" {')
    assert lines.index('extern "C" {') < lines.index('#include "api_setup.inc"') < lines.index('#include "api_inspect.inc"') < lines.index("}")
    assert lines[-1] == '#include "posterior_host.inc"'


def test_the_fragments_in_their_order():
    quoted = re.findall(r'^\s*#\s*include\s*"([^"]+\.inc)"', _code(_read("gvi_hip.hip")), re.M)
    assert quoted == FRAGMENTS


def test_every_fragment_is_on_the_list_and_included_once():
    on_disk = sorted(name for name in os.listdir(CSRC) if name.endswith(".inc"))
    assert on_disk == sorted(FRAGMENTS + [DATA, TIMING])
    for name in FRAGMENTS:
        assert _includers(name) == ["gvi_hip.hip"], name
    assert _includers(TIMING) == ["launch_factor.inc"]


def test_no_fragment_outgrows_a_sitting():
    sizes = {name: _read(name).count("\n") for name in sorted(os.listdir(CSRC)) if name.endswith(".inc")}
    print("    lines per fragment:", sizes)
    assert max(sizes.values()) <= MAX_LINES, sizes
