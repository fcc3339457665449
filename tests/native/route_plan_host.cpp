// route_plan_host.cpp — TEST ONLY: prints the launch plan of pxb_run_device
// (csrc/route_plan.h, csrc/ev_layouts.h) so that routing is checked without a GPU:
//   route_plan_host P N loss delay crash skew cap randomize ticks [hook ...]
//   route_plan_host sweep
// A hook is one of no_ev no_ff1 no_ffp no_split no_tight no_lg2 no_lgs, or
// bail_cap=K.  One line per plan: the plan as route_plan returns it, then what
// route_resolve makes of it when the first stage fits no more blocks than the
// second (u_*).  `sweep` prints the plan of every config and single hook of
// tests/test_route_plan.py's exhaustive sweep, each behind its config and hook.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cloud-haskell-paxos_amd/csrc/route_plan.h"

using namespace pxb;

static const char* const HOOKS[] = {"none", "no_ev", "no_ff1", "no_ffp", "no_split", "no_tight", "no_lg2", "no_lgs",
                                    "bail_cap=3"};

static bool set_hook(RouteHooks& h, const char* s) {
  bool* const f[] = {nullptr, &h.no_ev, &h.no_ff1, &h.no_ffp, &h.no_split, &h.no_tight, &h.no_lg2, &h.no_lgs};
  for (int i = 1; i < 8; ++i)
    if (!strcmp(s, HOOKS[i])) return *f[i] = true;
  if (!strncmp(s, "bail_cap=", 9)) return h.bail_cap = atoi(s + 9), true;
  return !strcmp(s, "none");
}

static void print_stage(const char* name, RouteStage s, const pxb_config* c) {
  printf(" %s=%u,%u,%d built=%d serves=%d", name, s.pm, c->n_acceptors, s.layout, (int)ev::layout_built(s.layout, s.pm),
         (int)ev::layout_serves(s.layout, c));
}

static void print_plan(const pxb_config* c, const RouteHooks& h) {
  static const char* const KIND[] = {"GENERAL", "FF1", "FFP", "EV"};
  static const char* const TWO[] = {"NONE", "SPLIT", "TIGHT", "LG2"};
  const RoutePlan r = route_plan(c, h), u = route_resolve(r, 1, 1), t = route_resolve(r, 2, 1);
  printf("kind=%s general=%d,%d two=%s cond=%d", KIND[r.kind], (int)r.logm, (int)r.ff, TWO[r.two_stage], (int)r.conditional);
  if (r.two_stage != TWO_NONE) print_stage("first", r.first, c);
  if (r.kind == ROUTE_EV) print_stage("second", r.second, c);
  printf(" chunk=%" PRIu64 " first_cap=%u cap=%u bail_word=%u", r.chunk, r.first_cap, r.cap, r.bail_word);
  // (a stage that fits more than the next keeps the plan as it is)
  const bool same = t.two_stage == r.two_stage && t.chunk == r.chunk && t.first_cap == r.first_cap && t.bail_word == r.bail_word;
  printf(" taken_same=%d u_two=%s u_chunk=%" PRIu64 " u_first_cap=%u u_bail_word=%u\n", (int)same, TWO[u.two_stage], u.chunk,
         u.first_cap, u.bail_word);
}

int main(int argc, char** argv) {
  pxb_config c{};
  c.crash_len_max = 1;
  c.tick_period = 4;
  if (argc == 2 && !strcmp(argv[1], "sweep")) {
    const uint32_t delays[] = {1, 4, 5, 8, 9, 15}, caps[] = {256, 512, 1024}, tickss[] = {1, 16};
    for (c.n_proposers = 1; c.n_proposers <= 3; ++c.n_proposers)
      for (c.n_acceptors = 2; c.n_acceptors <= 9; ++c.n_acceptors)
        for (uint32_t d : delays)
          for (uint32_t bits = 0; bits < 16; ++bits)
            for (uint32_t ticks : tickss)
              for (uint32_t cap : caps)
                for (const char* hook : HOOKS) {
                  c.delay_max = d;
                  c.loss_ppm = (bits & 1) ? 100000 : 0;
                  c.crash_ppm = (bits & 2) ? 100000 : 0;
                  c.skew_max = (bits & 4) ? 3 : 0;
                  c.flags = (bits & 8) ? PXB_CFG_RANDOMIZE : 0;
                  c.n_ticks = ticks;
                  c.step_cap = cap;
                  RouteHooks h{};
                  h.bail_cap = -1;
                  set_hook(h, hook);
                  printf("cfg=%u,%u,%u,%u,%u,%u,%u,%u,%u hook=%s ", c.n_proposers, c.n_acceptors, d, c.loss_ppm, c.crash_ppm,
                         c.skew_max, c.flags, ticks, cap, hook);
                  print_plan(&c, h);
                }
    return 0;
  }
  if (argc < 10) return 2;
  uint32_t* const f[] = {&c.n_proposers, &c.n_acceptors, &c.loss_ppm, &c.delay_max, &c.crash_ppm, &c.skew_max,
                         &c.step_cap, &c.flags, &c.n_ticks};
  for (int i = 0; i < 9; ++i) *f[i] = (uint32_t)strtoul(argv[1 + i], nullptr, 0);
  RouteHooks h{};
  h.bail_cap = -1;
  for (int i = 10; i < argc; ++i)
    if (!set_hook(h, argv[i])) return 2;
  print_plan(&c, h);
  return 0;
}
