// Host only, no device: conv_flow_wgrad_plan over its argument space, ragged length vectors included, to be built with the address and undefined-behaviour
// sanitizers on the host side and run on a CPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined
//         -I include -I comfy-rvc_amd/csrc tools/micro/flow_wgrad_plan_sweep.hip -o flow_wgrad_plan_sweep && ./flow_wgrad_plan_sweep
// Every accepted plan is checked for what the kernel and the finishing launch rely on: the stage prefix is the items' own (item b owns ceil(N[b] / 128) stages
// from first[b]), the splits cover every stage exactly once and none is empty, the grid covers the output, the partial images fit the bound.  Every argument
// set the planner documents as declined must be declined.  Prints the number of argument sets; exit status 0 when all hold.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../comfy-rvc_amd/csrc/conv_flow_wgrad.hip"

using namespace rvc;

static long long g_sets = 0, g_accepted = 0;
static void fail(const char* what, const ConvFlowWgradArgs& a) {
  std::fprintf(stderr, "FAILED: %s (B %d R %d R0 %d C %d k %d off0 %d gate %d N0 %d)\n", what, a.B, a.R, a.R0, a.C, a.k, a.off0, a.gate, a.N[0]);
  std::exit(1);
}
static void check(const ConvFlowWgradArgs& a) {
  ++g_sets;
  ConvFlowWgradPlan p;
  bool bad = a.B < 1 || a.B > kGenWgradMaxItems || a.R < 16 || a.R % 16 || a.R0 < 1 || a.R0 > a.R || a.C < 1 || a.k < 1 || a.k > 16 || a.off0 > 4096 || a.off0 < -4096 ||
             (a.gate != 0 && a.gate != 1) || (long long)a.R * a.C * a.k > (long long)kGenWgradPartFloats || (long long)a.C * a.k + 128 >= (1LL << 31);
  for (int b = 0; !bad && b < a.B; ++b) bad = a.N[b] < 1 || ((long long)a.N[b] + 128 + a.k + 4096) * 4 >= (1LL << 31);
  const bool ok = conv_flow_wgrad_plan(a, p);
  if (ok == bad) fail(bad ? "accepted what the planner documents as declined" : "declined a documented shape", a);
  if (!ok) return;
  ++g_accepted;
  long long total = 0;
  for (int b = 0; b < a.B; ++b) {
    if (p.a.first[b] != total) fail("first[] is not the prefix of the items' stages", a);
    total += ((long long)a.N[b] + 127) / 128;
  }
  if (p.a.first[a.B] != total || p.a.total != total) fail("total", a);
  if (p.splits < 1 || p.a.per < 1 || (long long)p.splits * p.a.per < total || (long long)(p.splits - 1) * p.a.per >= total) fail("the splits do not cover the stages once, none empty", a);
  const long long ncols = (long long)a.C * a.k;
  const int bn = p.bm == 32 ? 128 : 64;
  if ((p.bm != 128 && p.bm != 64 && p.bm != 32) || (long long)p.grid.x * bn < ncols || (long long)p.grid.y * p.bm < a.R || (int)p.grid.z != p.splits) fail("grid", a);
  if (p.part_floats != (size_t)p.splits * a.R * ncols || p.part_floats > kGenWgradPartFloats || p.splits > 32) fail("more partial images than the bound holds", a);
  if (p.lds != gather_pair_lds(p.bm, bn) || p.lds > 160 * 1024) fail("lds", a);
}

int main() {
  const int Rs[] = {0, 8, 16, 24, 32, 48, 64, 96, 128, 192, 384, 4096, 65536};
  const int Cs[] = {0, 1, 13, 96, 192, 4096, 1 << 20};
  const int ks[] = {0, 1, 5, 16, 17};
  const int offs[] = {-4097, -4096, -2, 0, 3, 4096, 4097};
  const long long Ns[] = {-1, 0, 1, 5, 127, 128, 129, 300, 5200, (1LL << 29) - 4300, 1LL << 29, (1LL << 31) - 1};
  unsigned rng = 12345u;
  auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
  for (int R : Rs) for (int C : Cs) for (int k : ks) for (int off0 : offs) for (int gate = -1; gate <= 2; ++gate) {
    // B and the lengths: every single length, uniform vectors, and ragged vectors drawn from the table
    for (int B : {-1, 0, 1, 2, 3, 16, 17}) {
      for (int mode = 0; mode < 4; ++mode) {
        ConvFlowWgradArgs a{};
        a.B = B; a.R = R; a.C = C; a.k = k; a.off0 = off0; a.gate = gate;
        a.R0 = mode == 3 ? R / 2 : R;
        for (int b = 0; b < kGenWgradMaxItems; ++b) {
          const long long n = mode == 0 ? Ns[next() % 12] : (mode == 1 ? 1 + (long long)(next() % 400) : (mode == 2 ? Ns[2 + next() % 7] : 3 + (long long)(next() % 38)));
          a.N[b] = (int)n;
        }
        check(a);
      }
    }
  }
  std::printf("conv_flow_wgrad_plan: %lld argument sets, %lld accepted, all checks hold\n", g_sets, g_accepted);
  return 0;
}
