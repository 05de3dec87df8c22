#!/usr/bin/env python
"""Launch census: which kernel instantiations does the CPU suite actually run?

The emulated build (tests/emu) registers every (kernel, template arguments) pair that a hipLaunchKernelGGL
names and marks it when it is launched.  This tool runs `pytest tests -m "not gpu"` in this process, snapshots
the launched set after every test, and writes profiles/kernel_census.txt: every instantiation, launched or
not, with the first test that launched it.  Instantiations that no argument and no debug knob can select are
listed under "unreachable" with the dispatch line that rules them out (UNREACHABLE below).

    python tools/kernel_census.py [-o FILE] [-j JOBS] [pytest arguments, default: tests]

Launches made by child processes of a test (the command-line tools) are not seen.
"""
import argparse
import ctypes
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# instantiation (regular expression over the census's spelling) -> the one-sentence proof that no argument selects it
UNREACHABLE = [
]


class Census:
    """pytest plugin: after each test, note which instantiations it was the first to launch."""

    def __init__(self, lib, harness):
        self.lib, self.h = lib, harness
        self.first = {}

    def pytest_runtest_logreport(self, report):
        if report.when != "teardown":
            return
        for name in self.h.census_launched(self.lib):
            self.first.setdefault(name, report.nodeid)


def unreachable_reason(name):
    for pat, why in UNREACHABLE:
        if re.fullmatch(pat, name):
            return why
    return None


def render(universe, first, seconds, args, jobs=1):
    never, unreach = [], []
    for n in sorted(universe):
        if n in first:
            continue
        why = unreachable_reason(n)
        (unreach if why else never).append((n, why))
    how = ("one process: a launched instantiation names the first test of the suite's order that launched it" if jobs <= 1 else
           "%d processes over the test modules: a launched instantiation names the lowest-sorting id among each process's first" % jobs)
    out = ["# Launch census of the emulated build: pytest %s" % " ".join(args), "# written by " + how,
           "# %d instantiations, %d launched, %d never launched, %d unreachable" % (len(universe), len(first), len(never), len(unreach)),
           "", "## never launched (%d)" % len(never)]
    out += [n for n, _ in never]
    out += ["", "## unreachable (%d): no argument and no debug knob selects these" % len(unreach)]
    out += ["%s  -- %s" % (n, why) for n, why in unreach]
    out += ["", "## launched (%d): instantiation <- first test that launched it" % len(first)]
    out += ["%s  <- %s" % (n, first[n]) for n in sorted(first)]
    return "\n".join(out) + "\n", never


def run_here(pytest_args):
    """pytest in this process -> (universe, {instantiation: first test id}, seconds, pytest's exit code)"""
    import pytest
    from tests import emu_harness
    from tests.emu import build as emu_build
    lib = ctypes.CDLL(emu_build.build())      # the same handle the tests' Emu() gets: one census per process
    universe = emu_harness.census_universe(lib)
    emu_harness.census_reset(lib)
    plugin = Census(lib, emu_harness)
    os.chdir(ROOT)
    t0 = time.time()
    rc = pytest.main(list(pytest_args) + ["-m", "not gpu"], plugins=[plugin])
    return universe, {n: t for n, t in plugin.first.items() if n in universe}, time.time() - t0, int(rc)


def run_split(jobs):
    """the test modules of tests/ dealt out to `jobs` child processes of this tool (largest first, to the least loaded), merged: of
    two tests that launched an instantiation, the one whose id sorts first is reported"""
    import json
    import subprocess
    import tempfile
    from tests.emu import build as emu_build
    emu_build.build()
    files = sorted((f for f in os.listdir(os.path.join(ROOT, "tests")) if f.startswith("test_") and f.endswith(".py")),
                   key=lambda f: -os.path.getsize(os.path.join(ROOT, "tests", f)))
    parts = [[] for _ in range(jobs)]
    load = [0] * jobs
    for f in files:
        k = load.index(min(load))
        parts[k].append(os.path.join("tests", f))
        load[k] += os.path.getsize(os.path.join(ROOT, "tests", f))
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for k, part in enumerate(parts):
            if part:
                out = os.path.join(tmp, "part%d.json" % k)
                procs.append((out, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--part", out] + part, cwd=ROOT)))
        universe, first, seconds, rc = set(), {}, 0.0, 0
        for out, p in procs:
            p.wait()
            r = json.load(open(out))
            universe |= set(r["universe"])
            seconds += r["seconds"]
            rc = rc or (0 if r["rc"] == 5 else r["rc"])        # 5: a part whose modules are all GPU tests collected nothing
            for n, t in r["first"].items():
                first[n] = min(first.get(n, t), t)
    return frozenset(universe), first, seconds, rc


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "kernel_census.txt"))
    ap.add_argument("-j", "--jobs", type=int, default=1, help="deal the test modules out to this many processes (the census is their union)")
    ap.add_argument("--part", help=argparse.SUPPRESS)          # a child of --jobs: write this JSON and no census file
    ap.add_argument("pytest_args", nargs="*", default=["tests"])
    a = ap.parse_args()
    if a.part:
        import json
        universe, first, seconds, rc = run_here(a.pytest_args)
        json.dump(dict(universe=sorted(universe), first=first, seconds=seconds, rc=rc), open(a.part, "w"))
        return 0
    t0 = time.time()
    universe, first, seconds, rc = run_split(a.jobs) if a.jobs > 1 else run_here(a.pytest_args)
    text, never = render(universe, first, seconds, a.pytest_args, a.jobs)
    with open(a.output, "w") as f:
        f.write(text)
    print("census: %d instantiations, %d launched, %d never launched (%d of them unreachable); pytest took %.0f s in all (%.0f s elapsed), exit %d -> %s"
          % (len(universe), len(first), len(universe) - len(first), len(universe) - len(first) - len(never), seconds, time.time() - t0, rc, a.output))
    return 1 if (never or rc) else 0


if __name__ == "__main__":
    sys.exit(main())
