"""The table of run-time switches (gaussianvi_amd/csrc/options.hpp) through a stand-alone program (tests/stubs/options_check.cpp),
as a plain build and under AddressSanitizer / UndefinedBehaviorSanitizer: what every environment variable and every option
name does to the Options of a context, the clamps and the refusals, and that include/gvi_hip.h lists exactly the table's names.
The environment reaches options_from_env through an injected look-up, never through the process environment."""
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stubs", "options_check.cpp")
BUILDS = {"plain": ["g++", "-O2", "-std=c++17", "-Wall"],
          "sanitized": ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

DEFAULTS = dict(warm_start=1, fuse_trial=2, target_waves=2048, mirror=1, split_flush=64, sreg_pipe=1, no_scost=0, orbit=1, fused=1,
                orbit_waves=4096, jacobi_tol=1e-34, chol_sqrt=1, chol_rowb=0, trust_table_degree=0, orbit_min_tiles=6, orbit_copies=8,
                pair_fuse=1, fuse_gather=1, side_solve=1, asm_on_load=1, chain_merge=1, chain_merge_fault=0, pipeline=1, spin_ms=2,
                safe_publish=0, sample_sweep=1, solve_lds=1, chain_wave=1, asm_dense=1, chain_pair=1)

# environment variable, its value -> the one field that leaves its default, and what it becomes
ENV_CASES = [
    ("GVI_ORBIT", 0, "orbit", 0), ("GVI_FUSED", 0, "fused", 0), ("GVI_ASM_ON_LOAD", 0, "asm_on_load", 0),
    ("GVI_PIPELINE", 0, "pipeline", 0), ("GVI_CHAIN_WAVE", 0, "chain_wave", 0), ("GVI_ASM_DENSE", 0, "asm_dense", 0),
    ("GVI_CHAIN_PAIR", 0, "chain_pair", 0), ("GVI_CHAIN_MERGE", 0, "chain_merge", 0), ("GVI_CHOL_ROWB", 1, "chol_rowb", 1),
    ("GVI_SIDE_SOLVE", 0, "side_solve", 0), ("GVI_NO_SCOST", 1, "no_scost", 1), ("GVI_SREG_PIPE", 0, "sreg_pipe", 0),
    ("GVI_MIRROR", 0, "mirror", 0), ("GVI_SAFE_PUBLISH", 1, "safe_publish", 1), ("GVI_SPIN_MS", 7, "spin_ms", 7),
    ("GVI_SPIN_MS", -3, "spin_ms", 0),
    ("GVI_NO_PAIR", 1, "pair_fuse", 0), ("GVI_NO_FUSE_GATHER", 1, "fuse_gather", 0),          # the two inverted names
    ("GVI_FUSE_TRIAL", 1, "fuse_trial", 1), ("GVI_FUSE_TRIAL", -1, "fuse_trial", 0), ("GVI_FUSE_TRIAL", 7, "fuse_trial", 2),
]
# ... and settings that leave everything at its default
ENV_NEUTRAL = [("GVI_NO_PAIR", 0), ("GVI_NO_FUSE_GATHER", 0), ("GVI_CHAIN_MERGE", 2),      # (2 is "on"; only OPTION value 2 sets the fault flag)
               ("GVI_SPECULATE", 0), ("GVI_WARM_START", 0), ("GVI_TARGET_WAVES", 1), ("GVI_SPLIT_FLUSH", 0), ("GVI_ORBIT_WAVES", 1),
               ("GVI_ORBIT_COPIES", 1), ("GVI_ORBIT_MIN_TILES", 1), ("GVI_ORBIT_STACK", 0), ("GVI_CHOL_SQRT", 0), ("GVI_JACOBI_TOL_EXP", -25)]

# option name, value -> field, what it becomes
SET_CASES = [
    ("split_flush", 3, "split_flush", 3), ("split_flush", -1, "split_flush", 0),
    ("sreg_pipe", 0, "sreg_pipe", 0), ("mirror", 0, "mirror", 0), ("pair_fuse", 0, "pair_fuse", 0), ("fuse_gather", 0, "fuse_gather", 0),
    ("side_solve", 0, "side_solve", 0), ("warm_start", 0, "warm_start", 0), ("no_scost", 1, "no_scost", 1),
    ("target_waves", 512, "target_waves", 512), ("target_waves", 0, "target_waves", 1),
    ("orbit", 0, "orbit", 0), ("fused", 0, "fused", 0), ("assemble_on_load", 0, "asm_on_load", 0), ("pipeline", 0, "pipeline", 0),
    ("chain_wave", 0, "chain_wave", 0), ("asm_dense", 0, "asm_dense", 0), ("chain_pair", 0, "chain_pair", 0),
    ("sample_sweep", 0, "sample_sweep", 0), ("solve_lds", 0, "solve_lds", 0), ("chain_merge", 0, "chain_merge", 0),
    ("chain_merge", 2, "chain_merge", 1),       # "on"; the fault flag of value 2 is gvi_set_option's own
    ("trust_table_degree", 1, "trust_table_degree", 1), ("safe_publish", 1, "safe_publish", 1), ("chol_sqrt", 0, "chol_sqrt", 0),
    ("chol_rowb", 1, "chol_rowb", 1), ("jacobi_tol_exp", -20, "jacobi_tol", math.pow(10.0, -20)), ("jacobi_tol_exp", -30, "jacobi_tol", math.pow(10.0, -30)),
    ("orbit_waves", 100, "orbit_waves", 100), ("orbit_waves", 0, "orbit_waves", 1),
    ("orbit_min_tiles", 3, "orbit_min_tiles", 3), ("orbit_min_tiles", 0, "orbit_min_tiles", 1),
    ("orbit_copies", 4, "orbit_copies", 4), ("orbit_copies", 0, "orbit_copies", 1), ("orbit_copies", 99, "orbit_copies", 16),
]
SET_REFUSED = [
    ("jacobi_tol_exp", -19, "jacobi_tol_exp must be <= -20 (threshold 10^value on squared magnitudes)"),
    ("orbit_stack", 1, "unknown option: orbit_stack"),
    ("dual_chain", 1, "unknown option: dual_chain"),
    ("fuse_trial", 1, "unknown option: fuse_trial"),          # environment only (the API is gvi_ngd_set_mode)
    ("spin_ms", 1, "unknown option: spin_ms"),
]
OPTION_NAMES = sorted({c[0] for c in SET_CASES})


def parse(line):
    head, _, body = line.partition(" | ")
    assert head == "ok", line
    out = {}
    for item in body.split():
        k, v = item.split("=")
        out[k] = float.fromhex(v) if k == "jacobi_tol" else int(v)
    return out


@pytest.fixture(scope="module", params=sorted(BUILDS))
def answers(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("options_" + request.param)
    exe = str(tmp / "options_check")
    r = subprocess.run(BUILDS[request.param] + [STUB, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cmds = ["rows", "defaults"]
    cmds += ["env %s %d" % c[:2] for c in ENV_CASES] + ["env %s %d" % c for c in ENV_NEUTRAL]
    cmds += ["set %s %d" % c[:2] for c in SET_CASES] + ["set %s %d" % c[:2] for c in SET_REFUSED]
    script = tmp / "commands.txt"
    script.write_text("\n".join(cmds) + "\n")
    r = subprocess.run([exe, str(script)], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cmds), r.stdout
    return dict(zip(cmds, lines))


def rows(answers):
    return [tuple(None if v == "-" else v for v in item.split(":")) for item in answers["rows"].split()[1:]]


def test_defaults(answers):
    assert parse(answers["defaults"]) == DEFAULTS


def test_every_environment_name_sets_its_field(answers):
    for env, value, field, want in ENV_CASES:
        assert parse(answers["env %s %d" % (env, value)]) == dict(DEFAULTS, **{field: want}), (env, value)
    for env, value in ENV_NEUTRAL:
        assert parse(answers["env %s %d" % (env, value)]) == DEFAULTS, (env, value)
    assert {e for _, e in rows(answers) if e} == {c[0] for c in ENV_CASES}


def test_every_option_name_is_accepted(answers):
    for name, value, field, want in SET_CASES:
        assert parse(answers["set %s %d" % (name, value)]) == dict(DEFAULTS, **{field: want}), (name, value)
    assert {n for n, _ in rows(answers) if n} == set(OPTION_NAMES)


def test_refusals(answers):
    for name, value, msg in SET_REFUSED:
        assert answers["set %s %d" % (name, value)] == "refused " + msg


def test_the_header_lists_the_table(answers):
    text = open(os.path.join(ROOT, "include", "gvi_hip.h")).read()
    table = text[text.index("A/B switches: the complete list"):text.index("Build-time only:")]
    first_column = {m.group(1) for m in re.finditer(r"^ \*   (GVI_[A-Z_]+) ", table, flags=re.M)}
    assert first_column == {e for _, e in rows(answers) if e} | {"GVI_SPGH_EXTENDED", "GVI_RCCL_PATH"}
    names = text[text.index(" * Names: ") + len(" * Names: "):]
    names = names[:names.index("*/")]
    listed = {n.strip() for n in names.replace("*", " ").replace(".", " ").split(",")}
    assert listed == {n for n, _ in rows(answers) if n}
    for env in ["GVI_JACOBI_TOL_EXP", "GVI_ORBIT_STACK"]:
        assert env not in text
