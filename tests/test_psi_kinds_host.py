"""The table of psi kinds (gaussianvi_amd/csrc/psi_kinds.hpp) through a stand-alone program (tests/stubs/psi_kinds_check.cpp),
as a plain build and under AddressSanitizer / UndefinedBehaviorSanitizer: the layout gvi_factors_add gives a set of every
kind, the shapes and parameter values it refuses with their exact texts, and the flags the other sites ask for.  Every
expected value below is written out from the documentation of the kinds in include/gvi_hip.h, not read back from the table."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stubs", "psi_kinds_check.cpp")
BUILDS = {"plain": ["g++", "-O2", "-std=c++17", "-Wall"],
          "sanitized": ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
OK, ERR_ARG = 0, 1

(RANGE_1D, QUAD_PRIOR, FIXED_PRIOR, HOST_CALLBACK, SDF_2D, SDF_2D_BODY, SDF_3D, SDF_3D_ARM, SDF_2D_SEG, SDF_3D_SEG, BOX,
 HALFSPACE) = range(12)

MSG_SEG = ("HINGE_SDF_*_SEG needs params_per_factor = 3 + J P (d + 1) with 1 <= J <= 8 check points "
           "(P = 2 for _2D_SEG, 3 for _3D_SEG)")
MSG_BOX = "HINGE_BOX needs params_per_factor = 4 d: [sigma | eps | lo | hi]"
MSG_HALFSPACE = "HINGE_HALFSPACE needs params_per_factor = J (d + 3) with 1 <= J <= 16 rows: [sigma (J) | eps (J) | b (J) | A (J x d)]"
MSG_SHORT = "psi_params missing or params_per_factor too small for this kind"

# (kind, d, params_per_factor) -> (status, m, J, need, message)
LAYOUTS = [
    ((RANGE_1D, 1, 5), (OK, 0, 0, 5, "")),                      # [y, mu_p, f*b, sig_r_sq, sig_p_sq]
    ((RANGE_1D, 1, 7), (OK, 0, 0, 5, "")),                      # a caller's stride may be longer than the block
    ((RANGE_1D, 1, 4), (ERR_ARG, 0, 0, 5, MSG_SHORT)),
    ((RANGE_1D, 2, 5), (ERR_ARG, 0, 0, 0, "RANGE_1D needs d == 1")),
    ((QUAD_PRIOR, 4, 8), (OK, 2, 0, 8, "")),                    # [Phi (n x n) | Qinv (n x n)], d = 2n
    ((QUAD_PRIOR, 3, 8), (ERR_ARG, 0, 0, 0, "QUAD_PRIOR needs even d")),
    ((FIXED_PRIOR, 3, 12), (OK, 3, 0, 12, "")),                 # [mu0 (d) | Kinv (d x d)]
    ((HOST_CALLBACK, 2, 0), (OK, 0, 0, 0, "")),
    ((SDF_2D, 2, 3), (OK, 0, 0, 3, "")),                        # [sigma, epsilon, radius]
    ((SDF_2D, 1, 3), (ERR_ARG, 0, 0, 0, "HINGE_SDF_2D needs d >= 2")),
    ((SDF_2D_BODY, 3, 6), (OK, 0, 0, 6, "")),                   # [sigma, epsilon, radius, slope, n_balls, L]
    ((SDF_2D_BODY, 2, 6), (ERR_ARG, 0, 0, 0, "HINGE_SDF_2D_BODY needs d >= 3")),
    ((SDF_3D, 3, 3), (OK, 0, 0, 3, "")),
    ((SDF_3D, 2, 3), (ERR_ARG, 0, 0, 0, "HINGE_SDF_3D needs d >= 3")),
    ((SDF_3D_ARM, 7, 2), (OK, 0, 0, 2, "")),                    # [sigma, epsilon]
    ((SDF_2D_SEG, 4, 3 + 1 * 2 * 5), (OK, 0, 1, 13, "")),       # 3 + J P (d + 1), P = 2
    ((SDF_2D_SEG, 4, 3 + 8 * 2 * 5), (OK, 0, 8, 83, "")),
    ((SDF_2D_SEG, 4, 3 + 9 * 2 * 5), (ERR_ARG, 0, 0, 0, MSG_SEG)),
    ((SDF_2D_SEG, 4, 12), (ERR_ARG, 0, 0, 0, MSG_SEG)),         # one double short
    ((SDF_2D_SEG, 4, 14), (ERR_ARG, 0, 0, 0, MSG_SEG)),         # one double long
    ((SDF_3D_SEG, 6, 3 + 1 * 3 * 7), (OK, 0, 1, 24, "")),       # P = 3
    ((BOX, 2, 8), (OK, 0, 0, 8, "")),                           # 4 d exactly
    ((BOX, 2, 7), (ERR_ARG, 0, 0, 0, MSG_BOX)),
    ((BOX, 2, 9), (ERR_ARG, 0, 0, 0, MSG_BOX)),
    ((HALFSPACE, 2, 16 * 5), (OK, 0, 16, 80, "")),              # J (d + 3) exactly
    ((HALFSPACE, 2, 17 * 5), (ERR_ARG, 0, 0, 0, MSG_HALFSPACE)),
    ((HALFSPACE, 2, 4), (ERR_ARG, 0, 0, 0, MSG_HALFSPACE)),
    ((-1, 2, 3), (ERR_ARG, 0, 0, 0, "unknown psi kind")),
    ((12, 2, 3), (ERR_ARG, 0, 0, 0, "unknown psi kind")),
]

# (kind, d, params_per_factor, K, values) -> (status, message).  BOX at d = 1: [sigma, eps, lo, hi]; HALFSPACE at d = 2,
# J = 1: [sigma, eps, b, a_0, a_1].  Two-factor cases carry the offending value in the SECOND block.
GOOD_BOX = "1 0.1 -1 1"
GOOD_HS = "1 0.1 2 1 0"
PARAMS = [
    ((BOX, 1, 4, 1, GOOD_BOX), (OK, "")),
    ((BOX, 1, 4, 2, GOOD_BOX + " -1 0 0 1"), (ERR_ARG, "HINGE_BOX: sigma must be finite and >= 0")),
    ((BOX, 1, 4, 1, "inf 0 0 1"), (ERR_ARG, "HINGE_BOX: sigma must be finite and >= 0")),
    ((BOX, 1, 4, 1, "1 inf 0 1"), (ERR_ARG, "HINGE_BOX: eps must be finite")),
    ((BOX, 1, 4, 1, "1 0 nan 1"), (ERR_ARG, "HINGE_BOX: NaN limit")),
    ((BOX, 1, 4, 1, "1 0 0 nan"), (ERR_ARG, "HINGE_BOX: NaN limit")),
    ((BOX, 1, 4, 1, "1 0 1 1"), (ERR_ARG, "HINGE_BOX: lo must be below hi (lo = -inf / hi = +inf switch a side off)")),
    ((BOX, 1, 4, 1, "1 0 inf inf"), (ERR_ARG, "HINGE_BOX: lo must be below hi (lo = -inf / hi = +inf switch a side off)")),
    ((BOX, 1, 4, 1, "1 0 -inf 1"), (OK, "")),
    ((BOX, 1, 4, 1, "1 0 -inf inf"), (OK, "")),
    ((BOX, 1, 4, 1, "null"), (ERR_ARG, MSG_SHORT)),
    ((HALFSPACE, 2, 5, 1, GOOD_HS), (OK, "")),
    ((HALFSPACE, 2, 5, 1, "nan 0 0 1 0"), (ERR_ARG, "HINGE_HALFSPACE: NaN in the parameter block")),
    ((HALFSPACE, 2, 5, 2, GOOD_HS + " 1 0 0 1 nan"), (ERR_ARG, "HINGE_HALFSPACE: NaN in the parameter block")),
    ((HALFSPACE, 2, 5, 1, "-1 0 0 1 0"), (ERR_ARG, "HINGE_HALFSPACE: sigma must be finite and >= 0")),
    ((HALFSPACE, 2, 5, 1, "1 -inf 0 1 0"), (ERR_ARG, "HINGE_HALFSPACE: eps must be finite")),
    ((HALFSPACE, 2, 5, 1, "1 0 inf 1 0"), (ERR_ARG, "HINGE_HALFSPACE: b must be finite")),
    ((HALFSPACE, 2, 5, 1, "1 0 0 1 inf"), (ERR_ARG, "HINGE_HALFSPACE: A must be finite")),
    ((HALFSPACE, 2, 5, 1, "1 0 0 0 0"), (ERR_ARG, "HINGE_HALFSPACE: an active row (sigma > 0) needs a non-zero normal a_j")),
    ((HALFSPACE, 2, 5, 1, "0 0 0 0 0"), (OK, "")),
    ((RANGE_1D, 1, 5, 1, "null"), (ERR_ARG, MSG_SHORT)),
    ((RANGE_1D, 1, 5, 1, "nan nan nan nan nan"), (OK, "")),     # only the limit kinds check values
    ((HOST_CALLBACK, 2, 0, 3, "null"), (OK, "")),
]

# what include/gvi_hip.h says of each kind: it keeps its block for the device psi (every kind but the two priors, whose
# operands are built on the host, and the host callback), reads the 2-D / 3-D grid, needs the arm model, has a clearance
# (the hinge kinds), has a closed form (gvi_factors_set_closed_form) and is created in it, is a sum of squares, has no device psi
FLAGS = {
    RANGE_1D: {"raw"},
    QUAD_PRIOR: {"sumsq", "closed"},
    FIXED_PRIOR: {"sumsq", "closed"},
    HOST_CALLBACK: {"no_device"},
    SDF_2D: {"raw", "sdf2d", "sdf", "clearance"},
    SDF_2D_BODY: {"raw", "sdf2d", "sdf", "clearance"},
    SDF_3D: {"raw", "sdf3d", "sdf", "clearance"},
    SDF_3D_ARM: {"raw", "sdf3d", "sdf", "arm", "clearance"},
    SDF_2D_SEG: {"raw", "sdf2d", "sdf", "clearance"},
    SDF_3D_SEG: {"raw", "sdf3d", "sdf", "clearance"},
    BOX: {"raw", "clearance", "closed", "closed_default"},
    HALFSPACE: {"raw", "clearance", "closed", "closed_default"},
    -1: set(),
    12: set(),
}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def answers(request, tmp_path_factory):
    """every command of this module through one run of the program -> the answer lines, by command line"""
    tmp = tmp_path_factory.mktemp("psi_kinds_" + request.param)
    exe = str(tmp / "psi_kinds_check")
    r = subprocess.run(BUILDS[request.param] + [STUB, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cmds = ["layout %d %d %d" % c for c, _ in LAYOUTS]
    cmds += ["params %d %d %d %d %s" % c for c, _ in PARAMS]
    cmds += ["flags %d" % k for k in FLAGS]
    script = tmp / "commands.txt"
    script.write_text("\n".join(cmds) + "\n")
    r = subprocess.run([exe, str(script)], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cmds), r.stdout
    return dict(zip(cmds, lines))


def test_the_kinds_have_the_numbers_of_the_header():
    text = open(os.path.join(ROOT, "include", "gvi_hip.h")).read()
    for name, value in [("RANGE_1D", RANGE_1D), ("QUAD_PRIOR", QUAD_PRIOR), ("FIXED_PRIOR", FIXED_PRIOR), ("HOST_CALLBACK", HOST_CALLBACK),
                        ("HINGE_SDF_2D", SDF_2D), ("HINGE_SDF_2D_BODY", SDF_2D_BODY), ("HINGE_SDF_3D", SDF_3D), ("HINGE_SDF_3D_ARM", SDF_3D_ARM),
                        ("HINGE_SDF_2D_SEG", SDF_2D_SEG), ("HINGE_SDF_3D_SEG", SDF_3D_SEG), ("HINGE_BOX", BOX), ("HINGE_HALFSPACE", HALFSPACE)]:
        assert f"GVI_PSI_{name} = {value}" in text, name


@pytest.mark.parametrize("case", range(len(LAYOUTS)), ids=["%d-d%d-ppf%d" % c for c, _ in LAYOUTS])
def test_layout(answers, case):
    (kind, d, ppf), (status, m, J, need, msg) = LAYOUTS[case]
    got = answers["layout %d %d %d" % (kind, d, ppf)]
    head, _, text = got.partition(" | ")
    assert head.split()[0] == "layout" and int(head.split()[1]) == status, got
    assert text == msg, got
    if status == OK:
        assert [int(v) for v in head.split()[2:]] == [m, J, need], got


@pytest.mark.parametrize("case", range(len(PARAMS)), ids=["%d-%s" % (c[0], c[4].replace(" ", "_")) for c, _ in PARAMS])
def test_parameter_values(answers, case):
    cmd, (status, msg) = PARAMS[case]
    got = answers["params %d %d %d %d %s" % cmd]
    assert got == "params %d | %s" % (status, msg)


def test_flags(answers):
    for kind, want in FLAGS.items():
        got = answers["flags %d" % kind].split()
        assert got[:2] == ["flags", str(kind)] and set(got[2:]) == want, (kind, got)
