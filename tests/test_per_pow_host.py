"""``libm_pow`` of csrc/per_pow.hpp against the C library's pow, on the host and without a GPU: a stand-alone
program (tests/support/per_pow_host.cpp) built with a host compiler the way ``PER_FLAGS`` builds the device code -- no
contraction, every ``fma()`` a hardware fused multiply-add -- evaluates the arguments of tests/support/pow_cases.py, and
``math.pow`` (the C library's, the function the numpy twin of the sum tree calls) must give the same bits for every covered one."""
import math
import os
import platform
import shutil
import subprocess

import numpy as np
import pytest

from support import pow_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "support", "per_pow_host.cpp")


def compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma" in line for line in f)
    except OSError:
        return False


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = compiler()
    if cxx is None:
        pytest.skip("no C++ compiler on PATH (CXX, c++, g++, clang++)")
    exe = str(tmp_path_factory.mktemp("per_pow") / "per_pow_host")
    flags = ["-O2", "-std=c++17", "-ffp-contract=off"]
    if platform.machine() in ("x86_64", "AMD64") and has_fma():
        flags.append("-mfma")           # aarch64 has the instruction in its base set
    r = subprocess.run([cxx, *flags, "-o", exe, SOURCE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def evaluated(program, tmp_path_factory):
    """(x, y, libm_pow's values, covered flags) of the whole argument set, one run of the program"""
    x, y = pow_cases.host_arguments()
    d = tmp_path_factory.mktemp("per_pow_io")
    np.stack([x, y], axis=1).astype("<f8").tofile(str(d / "in.bin"))
    r = subprocess.run([program, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.fromfile(str(d / "out.bin"), dtype=[("v", "<f8"), ("ok", "<u8")])
    assert len(out) == len(x)
    return x, y, out["v"].copy(), out["ok"] == 1


def test_the_arguments_reach_every_table_entry_and_every_way_out():
    x, y = pow_cases.host_arguments()
    x2, y2 = pow_cases.host_arguments()
    assert np.array_equal(x.view(np.uint64), x2.view(np.uint64)) and np.array_equal(y.view(np.uint64), y2.view(np.uint64))
    c = pow_cases.census(x, y)
    print(f"{len(x)} arguments, {int(c['covered'].sum())} covered; kinds {c['kinds']}")
    assert int(c["covered"].sum()) >= 10 ** 6
    assert c["log_intervals"] == list(range(128)) and c["exp_entries"] == list(range(128))
    for kind in ("tiny", "huge", "x_zero", "x_subnormal", "y_zero", "y_neg_zero"):
        assert c["kinds"][kind] >= 1, kind
    where = lambda xv, yv: np.flatnonzero((x == xv) & (y == yv) & (np.signbit(y) == np.signbit(yv)))
    kind_at = lambda xv, yv: {pow_cases.KIND_NAMES[k] for k in c["kind"][where(xv, yv)]}
    assert kind_at(1.0, 0.3) == {"tiny"} and kind_at(1.0 + 2.0 ** -52, 1e-3) == {"tiny"}
    assert kind_at(0.999, 1e6) == {"huge"} and kind_at(0.0, 1e6) == {"x_zero"} and kind_at(1e-310, 0.6) == {"x_subnormal"}
    assert kind_at(1.5, 0.0) == {"y_zero"} and kind_at(0.25, -0.0) == {"y_neg_zero"}
    # the sweep of tests/test_gpu_per.py: every (alpha, epsilon) alone reaches all log intervals, together all exp entries
    td, entries = pow_cases.td_errors(), set()
    assert len(td) == 4096 and (td == 0).sum() == 1 and (td == 1).sum() == 1 and (td < 0).sum() > 2000
    for alpha, epsilon in pow_cases.SWEEP:
        cs = pow_cases.census(*pow_cases.priority_arguments(td, alpha, epsilon))
        assert cs["log_intervals"] == list(range(128)), (alpha, epsilon)
        entries |= set(cs["exp_entries"])
    assert entries == set(range(128))


def test_libm_pow_equals_the_c_library_bit_for_bit(evaluated):
    x, y, v, ok = evaluated
    c = pow_cases.census(x, y)
    # the covered range is the one the header states: the program's flag equals the census's, argument by argument
    assert np.array_equal(ok, c["covered"]), np.flatnonzero(ok != c["covered"])[:8]
    idx = np.flatnonzero(ok)
    want = np.array([math.pow(a, b) for a, b in zip(x[idx].tolist(), y[idx].tolist())])
    bad = idx[v[idx].view(np.uint64) != want.view(np.uint64)]
    print(f"{len(idx)} covered arguments of {len(x)}: {len(bad)} differ from math.pow")
    assert len(idx) >= 10 ** 6
    assert len(bad) == 0, [(float(x[i]).hex(), float(y[i]).hex(), float(v[i]).hex(), math.pow(x[i], y[i]).hex()) for i in bad[:4]]
    # the early return is 1 + y log x rounded: 1, or its neighbour
    tiny = c["kind"] == pow_cases.TINY
    assert tiny.sum() > 1000 and np.all(np.abs(v[tiny] - 1.0) <= 2.0 ** -52)
