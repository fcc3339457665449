"""The staging carve (csrc/stage_plan.h) on the CPU: tests/native/stage_plan_host.cpp,
built with -Wall -Werror and again under the address and undefined-behaviour
sanitizers, checks the properties (256-byte alignment, ascending offsets that
do not overlap, empty regions that take nothing, the padded total, overflow
marking the plan invalid); and the offsets of the region lists of
pxb_run_scripted and pxb_shrink_batch equal the sums those functions spelled
out by hand before they were planned."""
import os
import subprocess

import pytest

import pxb

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "stage_plan_host.cpp")
DEPS = [SRC, os.path.join(HERE, "..", "cloud-haskell-paxos_amd", "csrc", "stage_plan.h")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def _bin(name, flags):
    out = os.path.join(HERE, "native", "_build", name)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        tmp = "%s.%d" % (out, os.getpid())
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, "-o", tmp, SRC], check=True)
        os.replace(tmp, out)
    return out


BUILDS = {"plain": ("stage_plan_host", []), "sanitized": ("stage_plan_host_san", SAN)}


@pytest.mark.parametrize("build", list(BUILDS))
def test_plan_properties(build):
    r = subprocess.run([_bin(*BUILDS[build]), "check"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


def pad256(b):
    return (b + 255) & ~255


def by_hand(sizes):
    """Offsets and total of regions of these byte sizes, each padded to 256, summed as the code before did."""
    offs, at = [], 0
    for b in sizes:
        offs.append(at)
        at += pad256(b)
    return offs + [at]


P, N, COUNT, DEPTH = 2, 5, 130, 8


def stride():
    # docs/SEMANTICS.md §10: a 16-byte head, N 4-byte windows, 2 P N links of depth entries, padded to 8
    want = (16 + 4 * N + 2 * P * N * DEPTH + 7) & ~7
    cfg = pxb.Config(seed=1, n_proposers=P, n_acceptors=N)
    assert pxb.script_stride(cfg, DEPTH) == want
    return want


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("form", ["scripted", "shrink"])
def test_offsets_equal_the_hand_written_sums(build, form):
    s = stride()
    if form == "scripted":      # rows_b + out_b + dig_b + acc_b + st_b + sent_b
        want = by_hand([COUNT * s, COUNT * 16, COUNT * N * 4, COUNT * N * 16, COUNT * 4, COUNT * 2 * P * N * 2])
    else:                       # rows_b + ids_b + 3 w_b + sent_b + res_b + sig_b
        want = by_hand([COUNT * s, COUNT * 8, COUNT * 4, COUNT * 4, COUNT * 4, COUNT * 2 * P * N * 2, COUNT * 16, COUNT * 8])
    out = subprocess.run([_bin(*BUILDS[build]), form, str(P), str(N), str(COUNT), str(DEPTH), str(s)],
                         capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out[:-1]] == want and out[-1] == "1"
