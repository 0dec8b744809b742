"""CPU checks of csrc/plan_switches.h - the one table of the launch plan's developer switches, the struct they resolve to and the
resolver - compiled into a stand-alone program with AddressSanitizer and UBSan, once as the shipped library sees it and once as a
`make DEV=1` build does (-DCONAN_DEV_SWITCHES).  The program resolves each dev_plan text it is given and prints every field; the
value spellings asserted here are the ones the library's read sites had before the table existed (tests and scripts depend on them)."""
import os
import re
import shutil
import subprocess

import pytest

from conan_amd import _lib

CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
TOOLS_README = os.path.join(os.path.dirname(os.path.dirname(_lib.LIB_PATH)), "tools", "README.md")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "plan_switches.h"

static const char* fake_env(const char* name) { return strcmp(name, "CONAN_TALL_MAXT") == 0 ? "5" : nullptr; }

// usage: prog [--setenv NAME=value]... [--fake-env] (--table | TEXT...)   ("NULL" stands for a null dev_plan)
int main(int argc, char** argv) {
  int a = 1;
  bool fake = false;
  for (; a < argc; ++a) {
    if (strcmp(argv[a], "--setenv") == 0 && a + 1 < argc) {
      const std::string kv(argv[++a]);
      setenv(kv.substr(0, kv.find('=')).c_str(), kv.substr(kv.find('=') + 1).c_str(), 1);
    } else if (strcmp(argv[a], "--fake-env") == 0) fake = true;
    else break;
  }
  if (a < argc && strcmp(argv[a], "--table") == 0) {
    for (const plan::Row& r : plan::kRows) printf("| `%s` | %s | %d | %s | %s |\n", r.name, plan::rule_text(r.rule), r.def, r.dev_only ? "`DEV`" : "all", r.what);
    return 0;
  }
  for (; a < argc; ++a) {
    try {
      const plan::PlanSwitches sw = strcmp(argv[a], "NULL") == 0 ? plan::resolve(nullptr) : (fake ? plan::resolve(argv[a], fake_env) : plan::resolve(argv[a]));
      for (const plan::Row& r : plan::kRows) {
        if (r.rule == plan::Rule::CfgList) { printf("%s=", r.name); for (int u = 0; u < plan::kMaxUps; ++u) printf("%d%s", sw.ups_cfg[u], u + 1 < plan::kMaxUps ? "," : " "); }
        else printf("%s=%d ", r.name, r.b ? (int)(sw.*r.b) : sw.*r.i);
      }
      printf("GRID256=%d GRID64=%d\n", plan::mega_grid(sw, 256), plan::mega_grid(sw, 64));      // the decoder launch's workgroups on 256 / 64 CUs
    } catch (const std::invalid_argument& e) { printf("ERROR %s\n", e.what()); }
  }
  return 0;
}
"""

SHIPPED = ("RESERVE_CUS", "ROWCONV", "RB_NOMERGE", "RB_NOLIMB", "FENCED", "DEC_MEGA", "MEGA_GRID", "FRONT_CUSTRIDE", "EMF_CUSTRIDE", "MEGA_GS", "MEGA_NARROW",
           "MEGA_NOL2", "FRONT_PRIO", "RB_UNFUSED", "RB_FUSED", "RB_PAIR", "RB_NOPAIR", "RP_MIN_SLOTS", "UPS_CFG", "EMF_CLUSTER", "EMF_UNFUSED", "NO_TALL",
           "TALL_MAXT")
DEV_ONLY = ("NO_TAILSPLIT", "SK_MIN", "MEGA_STAMPS", "MEGA_XCD_PAD", "MEGA_NOFFN", "CL_SHAPE", "RC_NOKSPLIT", "RC_WIDE_MIN", "SKIP_STAGE", "EMF_HOLD", "MEGA_LAYOUT")
NOT_FORCED = [-1] * 8
DEFAULTS = dict(RESERVE_CUS=0, ROWCONV=1, RB_NOMERGE=0, RB_NOLIMB=0, FENCED=0, DEC_MEGA=1, MEGA_GRID=0, FRONT_CUSTRIDE=0, EMF_CUSTRIDE=0, MEGA_GS=8, MEGA_NARROW=1,
                MEGA_NOL2=0, MEGA_LAYOUT=0, FRONT_PRIO=0, RB_UNFUSED=0, RB_FUSED=0, RB_PAIR=0, RB_NOPAIR=0, RP_MIN_SLOTS=16, UPS_CFG=NOT_FORCED, EMF_CLUSTER=0,
                EMF_UNFUSED=0, NO_TALL=0, TALL_MAXT=32, NO_TAILSPLIT=0, SK_MIN=12, MEGA_STAMPS=0, MEGA_XCD_PAD=0, MEGA_NOFFN=0, CL_SHAPE=-1, RC_NOKSPLIT=0,
                RC_WIDE_MIN=1024, SKIP_STAGE=0, EMF_HOLD=0, GRID256=128, GRID64=128)


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    """the program as the shipped library / as a DEV build compiles the header"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not present")
    d = tmp_path_factory.mktemp("plan_switches")
    src = d / "plan_switches_check.cpp"
    src.write_text(PROGRAM)
    out = {}
    for name, extra in (("shipped", []), ("dev", ["-DCONAN_DEV_SWITCHES"])):
        exe = d / ("check_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra, "-I", CSRC, str(src), "-o", str(exe)],
                       check=True)
        out[name] = str(exe)
    return out


def resolve(exe, *texts, pre=()):
    """-> per text the resolved fields {NAME: int, UPS_CFG: [int] * 8}, or the error message (str)"""
    r = subprocess.run([exe, *pre, *texts], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(texts), r.stdout
    out = []
    for line in lines:
        if line.startswith("ERROR "):
            out.append(line[6:])
            continue
        d = {}
        for item in line.split():
            k, v = item.split("=")
            d[k] = [int(x) for x in v.split(",")] if k == "UPS_CFG" else int(v)
        out.append(d)
    return out


def changed(d):
    assert isinstance(d, dict), d
    assert sorted(d) == sorted(DEFAULTS)
    return {k: v for k, v in d.items() if v != DEFAULTS[k]}


@pytest.mark.parametrize("build", ["shipped", "dev"])
def test_defaults(progs, build):
    for d in resolve(progs[build], "NULL", "", " ", ";", " ; ;; "):
        assert d == DEFAULTS


@pytest.mark.parametrize("build", ["shipped", "dev"])
def test_value_spellings_are_the_read_sites(progs, build):
    ups = lambda *v: list(v) + [-1] * (8 - len(v))
    cases = [
        # presence switches: any value, "0" included, switches the feature
        ("NO_TALL=0", dict(NO_TALL=1)), ("RB_NOMERGE=0", dict(RB_NOMERGE=1)), ("RB_PAIR=0", dict(RB_PAIR=1)), ("MEGA_NOL2=0", dict(MEGA_NOL2=1)),
        ("RB_NOLIMB=", dict(RB_NOLIMB=1)), ("RB_UNFUSED=x;RB_FUSED=no;RB_NOPAIR=1", dict(RB_UNFUSED=1, RB_FUSED=1, RB_NOPAIR=1)),
        # first character '1'
        ("FENCED=1", dict(FENCED=1)), ("FENCED=2", {}), ("FENCED=0", {}), ("FENCED=10", dict(FENCED=1)), ("FENCED=", {}), ("EMF_UNFUSED=1", dict(EMF_UNFUSED=1)),
        ("EMF_UNFUSED=yes", {}),
        # first character '0'
        ("ROWCONV=1", {}), ("ROWCONV=0", dict(ROWCONV=0)), ("ROWCONV=", {}), ("ROWCONV=off", {}), ("DEC_MEGA=0", dict(DEC_MEGA=0)), ("DEC_MEGA=00", dict(DEC_MEGA=0)),
        ("DEC_MEGA=1", {}), ("MEGA_NARROW=0", dict(MEGA_NARROW=0)), ("MEGA_NARROW=2", {}),
        # integers
        ("RESERVE_CUS=24", dict(RESERVE_CUS=24)), ("RESERVE_CUS=-3", dict(RESERVE_CUS=-3)), ("RESERVE_CUS=x", {}), ("RP_MIN_SLOTS=4", dict(RP_MIN_SLOTS=4)),
        ("RP_MIN_SLOTS=", dict(RP_MIN_SLOTS=0)), ("TALL_MAXT=8", dict(TALL_MAXT=8)), ("TALL_MAXT=0", dict(TALL_MAXT=0)), ("FRONT_PRIO=-1", dict(FRONT_PRIO=-1)),
        ("FRONT_CUSTRIDE=2;EMF_CUSTRIDE=4", dict(FRONT_CUSTRIDE=2, EMF_CUSTRIDE=4)), ("EMF_CLUSTER=4", dict(EMF_CLUSTER=4)),
        # MEGA_GS: 4, 8 or 16, anything else ignored
        ("MEGA_GS=4", dict(MEGA_GS=4)), ("MEGA_GS=16", dict(MEGA_GS=16)), ("MEGA_GS=8", {}), ("MEGA_GS=5", {}), ("MEGA_GS=0", {}), ("MEGA_GS=32", {}),
        # MEGA_GRID: positive values only, clamped to the CU count (GRID256 / GRID64: plan::mega_grid on 256 / 64 CUs); the default 128 is not clamped
        ("MEGA_GRID=64", dict(MEGA_GRID=64, GRID256=64, GRID64=64)), ("MEGA_GRID=0", {}), ("MEGA_GRID=-3", {}), ("MEGA_GRID=x", {}),
        ("MEGA_GRID=100000", dict(MEGA_GRID=100000, GRID256=256, GRID64=64)), ("MEGA_GRID=200", dict(MEGA_GRID=200, GRID256=200, GRID64=64)),
        # UPS_CFG: entry i for upsampler i, an empty entry forces nothing; the range check against the configuration count is the step's
        ("UPS_CFG=,5", dict(UPS_CFG=ups(-1, 5))), ("UPS_CFG=1", dict(UPS_CFG=ups(1))), ("UPS_CFG=0,1,2,3", dict(UPS_CFG=ups(0, 1, 2, 3))),
        ("UPS_CFG=3,", dict(UPS_CFG=ups(3))), ("UPS_CFG=", {}), ("UPS_CFG=,,7", dict(UPS_CFG=ups(-1, -1, 7))), ("UPS_CFG=99,-4,2", dict(UPS_CFG=ups(99, -4, 2))),
        ("UPS_CFG=1,2,3,4,5,6,7,0,1,2", dict(UPS_CFG=[1, 2, 3, 4, 5, 6, 7, 0])),
        # a bare name means NAME=1
        ("FENCED", dict(FENCED=1)), ("NO_TALL", dict(NO_TALL=1)), ("ROWCONV", {}), ("RESERVE_CUS", dict(RESERVE_CUS=1)), ("MEGA_GS", {}), ("UPS_CFG", dict(UPS_CFG=ups(1))),
        # trimming, empty items, a trailing ';'
        ("  FENCED=1  ", dict(FENCED=1)), ("FENCED=1;", dict(FENCED=1)), ("FENCED=1;;NO_TALL", dict(FENCED=1, NO_TALL=1)), (" RB_NOMERGE=1 ; FENCED=1 ", dict(RB_NOMERGE=1, FENCED=1)),
        (";;TALL_MAXT=8;", dict(TALL_MAXT=8)),
        # a name given twice: the last one holds
        ("MEGA_GRID=64;MEGA_GRID=0", {}), ("TALL_MAXT=8;TALL_MAXT=16", dict(TALL_MAXT=16)), ("FENCED=1;FENCED=2", {}),
    ]
    got = resolve(progs[build], *[t for t, _ in cases])
    for (text, want), d in zip(cases, got):
        assert changed(d) == want, text


@pytest.mark.parametrize("build", ["shipped", "dev"])
def test_unknown_names_are_rejected_by_name(progs, build):
    for text, name in (("BOGUS=2", "BOGUS"), ("FENCED=1;NOPE", "NOPE"), ("fenced=1", "fenced"), ("FENCED =1", "FENCED "), ("CONAN_FENCED=1", "CONAN_FENCED"), ("=1", ""),
                       ("MEGA_SINGLE=0", "MEGA_SINGLE"), ("MEGA_BLK=1", "MEGA_BLK")):
        (msg,) = resolve(progs[build], text)
        assert msg == "conan_streams_opts.dev_plan: unknown switch '%s'" % name, text


def test_shipped_build_has_no_dev_only_name_and_reads_no_environment(progs):
    for name in DEV_ONLY:
        for text in (name, name + "=1", "FENCED=1;" + name + "=m"):
            (msg,) = resolve(progs["shipped"], text)
            assert msg == "conan_streams_opts.dev_plan: unknown switch '%s'" % name
    # the environment is never consulted, through the default lookup (the program calls setenv first) or through one passed in
    env = ["--setenv", "CONAN_EMF_UNFUSED=1", "--setenv", "CONAN_FENCED=1", "--setenv", "CONAN_NO_TALL=1", "--setenv", "CONAN_SKIP_STAGE=3", "--setenv", "CONAN_UPS_CFG=1,1"]
    a, b, c = resolve(progs["shipped"], "NULL", "", "RB_NOMERGE=1", pre=env)
    assert changed(a) == {} and changed(b) == {} and changed(c) == dict(RB_NOMERGE=1)
    assert changed(resolve(progs["shipped"], "", pre=["--fake-env"])[0]) == {}
    assert set(SHIPPED) | set(DEV_ONLY) | {"GRID256", "GRID64"} == set(DEFAULTS)


def test_dev_build_takes_dev_only_names_and_falls_back_to_the_environment(progs):
    cases = [("NO_TAILSPLIT=0", dict(NO_TAILSPLIT=1)), ("SK_MIN=2", dict(SK_MIN=2)), ("MEGA_STAMPS", dict(MEGA_STAMPS=1)), ("MEGA_XCD_PAD=1", dict(MEGA_XCD_PAD=1)),
             ("MEGA_NOFFN=1", dict(MEGA_NOFFN=1)), ("CL_SHAPE=2", dict(CL_SHAPE=2)), ("CL_SHAPE=", {}), ("CL_SHAPE=0", dict(CL_SHAPE=0)), ("RC_NOKSPLIT", dict(RC_NOKSPLIT=1)),
             ("RC_WIDE_MIN=512", dict(RC_WIDE_MIN=512)), ("SKIP_STAGE=3", dict(SKIP_STAGE=3)), ("EMF_HOLD=1", dict(EMF_HOLD=1)), ("MEGA_LAYOUT=m", dict(MEGA_LAYOUT=1)),
             ("MEGA_LAYOUT=member", dict(MEGA_LAYOUT=1)), ("MEGA_LAYOUT=g", {}), ("MEGA_LAYOUT", {})]
    for (text, want), d in zip(cases, resolve(progs["dev"], *[t for t, _ in cases])):
        assert changed(d) == want, text
    env = ["--setenv", "CONAN_EMF_UNFUSED=1", "--setenv", "CONAN_TALL_MAXT=8", "--setenv", "CONAN_NO_TALL=", "--setenv", "CONAN_UPS_CFG=,5", "--setenv", "CONAN_MEGA_GS=5",
           "--setenv", "CONAN_SKIP_STAGE=2", "--setenv", "EMF_HOLD=1", "--setenv", "CONAN_BOGUS=1"]
    from_env = dict(EMF_UNFUSED=1, TALL_MAXT=8, NO_TALL=1, UPS_CFG=[-1, 5] + [-1] * 6, SKIP_STAGE=2)
    a, b, c, e = resolve(progs["dev"], "NULL", "RB_PAIR=1", "TALL_MAXT=16;EMF_UNFUSED=0;UPS_CFG=2", "BOGUS=1", pre=env)
    assert changed(a) == from_env
    assert changed(b) == dict(from_env, RB_PAIR=1)
    assert changed(c) == dict(NO_TALL=1, SKIP_STAGE=2, TALL_MAXT=16, UPS_CFG=[2] + [-1] * 7)      # the text wins, value by value
    assert e == "conan_streams_opts.dev_plan: unknown switch 'BOGUS'"
    # ... through whatever lookup the caller passes
    x, y = resolve(progs["dev"], "", "TALL_MAXT=9", pre=["--fake-env"])
    assert changed(x) == dict(TALL_MAXT=5) and changed(y) == dict(TALL_MAXT=9)


def test_tools_readme_lists_the_table(progs):
    """tools/README.md carries a copy of the table (name, rule, default, builds, description): it is the header's, row for row"""
    r = subprocess.run([progs["shipped"], "--table"], capture_output=True, text=True, check=True)
    rows = r.stdout.splitlines()
    assert [re.match(r"\| `(\w+)` \|", x).group(1) for x in rows] == [re.match(r"\| `(\w+)` \|", x).group(1) for x in
                                                                   subprocess.run([progs["dev"], "--table"], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert sorted(re.match(r"\| `(\w+)` \|", x).group(1) for x in rows) == sorted(set(SHIPPED) | set(DEV_ONLY))
    readme = [x.rstrip() for x in open(TOOLS_README).read().splitlines()]
    listed = [x for x in readme if re.match(r"\| `[A-Z0-9_]+` \|", x)]
    assert listed == rows
