"""The per-lane state machine's lane-masked stores (csrc/paxos_ev.h,
PXB_EV_STORE_BACK 2): a lane that does not write a link, pool or payload word
stores nothing, instead of storing the old value back, and the loads that
only fed that store-back are gone.

A stand-alone host program (tests/native/ev_masked_store_host.cpp) runs the
lane over a recording accessor that has the masked stores, on the tight,
layout-6, slim P = 2, log-mode and slim P = 3 shapes, one pinned instance at a
time, and every instance is compared with the CPU oracle: result words,
digests, rounds, executes, messages, canonical bytes, and whether it is handed
on.  The accessor fails a masked store that leaves the wrong memory (a false
predicate must leave it as it was) and an acceptor op that takes a broadcast
payload nobody wrote since the instance started.  Every store site occurs
with its predicate true and false: a handler with one broadcast, with two (the
restart after an Execute) and with none; a first send that is a reply, one
that is a second copy, and none; and the hand-offs of a full request FIFO, a
full response FIFO and an empty pool.  The ids are those of
tests/test_ev_rare_paths.py (chosen over the first 20,000 instances of each
config).

There is no Philox variant to compare with philox_rk: LLVM already hoists
round 0's instance-constant product out of the iteration loop, so none was
added."""
import os
import subprocess

import numpy as np
import pytest

import oracle_c
import pxb

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ev_masked_store_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "ev_masked_store_host")
DEPS = [SRC] + [os.path.join(HERE, "..", "cloud-haskell-paxos_amd", "csrc", f)
                for f in ("paxos_ev.h", "paxos_ev_kernel.h", "paxos_device.h", "ev_layouts.h")] + [
                    os.path.join(HERE, "..", "include", "paxos_batch.h")]
# a record's words (ev_masked_store_host.cpp); regions of the masked stores
(RW_ID, RW_RES, RW_ROUNDS, RW_EXECS, RW_MSGS, RW_CANON, RW_BAILED, RW_PROBES, RW_ITERS, RW_FLAGS, RW_STEPS, RW_BC_NONE,
 RW_BC_ONE, RW_BC_TWO, RW_S1_REPLY, RW_S1_COPY, RW_S1_NONE, RW_ST_TRUE, RW_ST_FALSE, RW_ERR_STORE, RW_ERR_STALE,
 RW_N) = (0, 1, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 25, 30, 31, 32)
RG_REQ, RG_RSP, RG_POOL, RG_BRING = 0, 1, 2, 3
# the header's probe bits (paxos_ev.h)
EVB_RING, EVB_RFIFO, EVB_POOL, EVB_QFIFO = 1 << 16, 1 << 17, 1 << 18, 1 << 19


# The builds: the sites the library uses (the header's default), and every
# site (PXB_EV_ST_IF_SITES=63), so that the forms that are not the default stay
# exact too.
BUILDS = {"default": [], "all_sites": ["-DPXB_EV_ST_IF_SITES=63"]}


def program(build="default"):
    """The host program, built once (parallel workers: build, then rename)."""
    out = OUT + "_" + build
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        tmp = "%s.%d" % (out, os.getpid())
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", *BUILDS[build], "-o", tmp,
                        SRC], check=True)
        os.replace(tmp, out)
    return out


def config_hex(cfg):
    return bytes(cfg.to_c(0, 1 << 31)).hex()


def run_ids(cfg, layout, pm, ids, build="default"):
    """The program's records of the ids: {id: words}."""
    p = subprocess.run([program(build), "run", config_hex(cfg), str(layout), str(pm)] + [str(g) for g in ids],
                       capture_output=True, text=True)
    assert p.returncode == 0, "ev_masked_store_host rc=%d: %s" % (p.returncode, p.stderr[-400:])
    recs = {}
    for line in p.stdout.splitlines():
        r = np.array([int(x) for x in line.split()], np.uint64)
        assert len(r) == RW_N + cfg.n_acceptors
        r.setflags(write=False)
        recs[int(r[RW_ID])] = r
    assert sorted(recs) == sorted(ids)
    return recs


def bailed_ids(cfg, layout, pm, n):
    """The ids of 0 .. n - 1 that the shape hands on (the accessor's checks on: rc 4 if one fails)."""
    p = subprocess.run([program(), "bails", config_hex(cfg), str(layout), str(pm), str(n)],
                       capture_output=True, text=True)
    assert p.returncode == 0, "ev_masked_store_host rc=%d: %s" % (p.returncode, p.stderr[-400:])
    return [int(x) for x in p.stdout.split()]


LOG_CFG = pxb.Config(seed=0x1065, n_proposers=2, n_acceptors=5, loss_ppm=100000, delay_max=4, skew_max=3,
                     crash_ppm=200000, crash_len_max=12, crash_start_max=30, step_cap=1024, n_ticks=16, tick_period=4)
FIRST = list(range(96))
# config 5's instances drawn with three proposers: the two-proposer shape hands them on in init
P3_OF_FIRST = [1, 3, 6, 9, 15, 16, 19, 20, 22, 26, 28, 38, 39, 40, 41, 42, 43, 45, 46, 48, 53, 57, 59, 67, 73, 77, 78,
               79, 81, 82, 92, 93, 94]
# shape: layout, proposer capacity, config, ids beyond the first 96, the ids
# handed on, and the pinned hand-offs: cause -> id
SHAPES = {
    "tight": (7, 2, pxb.CONFIGS[4], [160, 246, 286, 369, 4524, 5133], [49, 67, 160, 246, 286, 369],
              dict(full_rfifo=49, empty_pool=67)),
    "layout6": (6, 2, pxb.CONFIGS[4], [160, 246, 2770, 4524, 10705], [2770, 10705], dict(empty_pool=2770)),
    "slim_p2": (5, 2, pxb.CONFIGS[5], [235, 721, 2751, 3971], P3_OF_FIRST + [235, 721, 2751, 3971],
                dict(full_rfifo=235, empty_pool=2751)),
    "log_p2": (4, 2, LOG_CFG, [], [], dict()),
    "slim_p3": (5, 3, pxb.CONFIGS[5], [984, 2029, 2390, 2409], [984, 2029, 2390, 2409],
                dict(empty_pool=2029, full_qfifo=2409)),
}
CAUSE = dict(full_rfifo=EVB_RFIFO, empty_pool=EVB_POOL, full_qfifo=EVB_QFIFO)
_recs = {}


def records(shape, build):
    """The program's records of the shape's ids, run once and left unchanged."""
    if (shape, build) not in _recs:
        layout, pm, cfg, extra, _, _ = SHAPES[shape]
        _recs[(shape, build)] = run_ids(cfg, layout, pm, FIRST + extra, build)
    return _recs[(shape, build)]


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_instance_matches_the_oracle(shape, build):
    _, _, cfg, _, handed_on, _ = SHAPES[shape]
    recs = records(shape, build)
    N = cfg.n_acceptors
    assert sorted(g for g in recs if recs[g][RW_BAILED]) == sorted(handed_on)      # the hand-off decision
    for g, r in recs.items():
        if r[RW_BAILED]:
            continue
        eres, edig, _, cnt = oracle_c.run_cpu(cfg, g, 1)
        assert list(r[RW_RES:RW_RES + 4]) == list(eres[0]), "instance %d: result words" % g
        assert list(r[RW_N:RW_N + N]) == list(edig[0]), "instance %d: digests" % g
        got = dict(rounds=int(r[RW_ROUNDS]), executes=int(r[RW_EXECS]), messages=int(r[RW_MSGS]),
                   canon_bytes=int(r[RW_CANON]), steps=int(r[RW_STEPS]),
                   panic=int(bool(int(r[RW_FLAGS]) & pxb.F_PANIC)), stuck=int(bool(int(r[RW_FLAGS]) & pxb.F_STUCK)),
                   divergence=int(bool(int(r[RW_FLAGS]) & pxb.F_LOG_DIVERGENCE)),
                   undecided=int(bool(int(r[RW_FLAGS]) & pxb.F_UNDECIDED)),
                   step_cap=int(bool(int(r[RW_FLAGS]) & pxb.F_STEP_CAP)))
        assert got == {k: cnt[k] for k in got}, "instance %d" % g


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_accessor_saw_no_wrong_store_and_no_stale_payload(shape, build):
    for g, r in records(shape, build).items():
        assert r[RW_ERR_STORE] == 0, "instance %d: a masked store left the wrong memory" % g
        assert r[RW_ERR_STALE] == 0, "instance %d: an acceptor op took a payload never written" % g


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_site_stores_and_skips(shape, build):
    """Each region's masked stores occur with the predicate true and false
    (the pool word's false case is the empty pool, a pinned hand-off), and so
    do the cases the sites exist for.  The default build masks the request
    links (the acceptor op) and the payloads (the broadcast); the other build
    the response links and the pool words too."""
    recs = records(shape, build)
    tot = sum(r.astype(np.int64) for r in recs.values())
    for rg in (RG_REQ, RG_BRING) + ((RG_RSP,) if build == "all_sites" else ()):
        assert tot[RW_ST_TRUE + rg] > 0 and tot[RW_ST_FALSE + rg] > 0, rg
    assert (tot[RW_ST_TRUE + RG_POOL] > 0) == (build == "all_sites")
    assert tot[RW_BC_NONE] > 0 and tot[RW_BC_ONE] > 0 and tot[RW_BC_TWO] > 0
    assert tot[RW_S1_REPLY] > 0 and tot[RW_S1_COPY] > 0 and tot[RW_S1_NONE] > 0
    # the payload stores come in pairs: one handler, two stores
    assert tot[RW_ST_TRUE + RG_BRING] >= tot[RW_BC_ONE] + 2 * tot[RW_BC_TWO]


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_each_pinned_hand_off_is_present(shape, build):
    recs = records(shape, build)
    for cause, g in SHAPES[shape][5].items():
        r = recs[g]
        assert r[RW_BAILED] and int(r[RW_PROBES]) & CAUSE[cause], "%s: instance %d" % (cause, g)


def test_the_shapes_have_every_hand_off():
    assert {"full_rfifo", "empty_pool", "full_qfifo"} <= {c for s in SHAPES.values() for c in s[5]}
