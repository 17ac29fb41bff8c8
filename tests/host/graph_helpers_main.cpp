// Host-only exercise of the graph helpers of csrc/rvc_internal.h (arena_passes, ZeroedBlock) with Arena::ensure / release over malloc / free: built with the host
// compiler and AddressSanitizer + UBSan by tests/test_graph_helpers_host.py, no HIP runtime linked.  Exit status 0, or 100 when a check failed.
#include "rvc_internal.h"

static size_t g_ensured = 0; static int g_ensures = 0;
namespace rvc {
void set_error(const std::string&) {}
void Arena::ensure(size_t bytes) {
  ++g_ensures; g_ensured = bytes;
  if (bytes <= cap) return;
  free(base); base = static_cast<char*>(malloc(bytes)); cap = bytes; ++gen;
}
void Arena::release() { free(base); base = nullptr; cap = 0; ++gen; }
}  // namespace rvc
using namespace rvc;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(100); } } while (0)

int main() {
  {  // arena_passes: the graph runs twice (dry, then real on the block the dry pass measured); ensure sees the dry pass's peak
    Arena A;
    A.peak = 1 << 20;      // left by an earlier, larger call
    int calls = 0; bool dry_seen[2] = {false, false}; float* real = nullptr;
    arena_passes(A, [&] {
      CHECK(calls < 2 && A.off == 0);
      dry_seen[calls++] = A.dry;
      float* a = A.alloc<float>(100);            // 400 -> 512 bytes
      const size_t mark = A.off;
      A.alloc<char>(1000);                       // a scoped temporary: 1024
      A.off = mark;
      float* b = A.alloc<float>(10);             // 256, inside the temporary's bytes
      if (!A.dry) { a[99] = 1.f; b[9] = 2.f; real = a; }
    });
    CHECK(calls == 2 && dry_seen[0] && !dry_seen[1] && !A.dry);
    CHECK(g_ensures == 1 && g_ensured == 512 + 1024 && A.peak == g_ensured && A.cap >= A.peak);
    CHECK(real == reinterpret_cast<float*>(A.base) && real[99] == 1.f);
    // a graph that throws in the dry pass, then one that throws in the real pass: dry is false afterwards, ensure not reached / reached once
    for (int bad = 0; bad < 2; ++bad) {
      int n = 0; bool thrown = false;
      g_ensures = 0;
      try { arena_passes(A, [&] { A.alloc<float>(8); if (n++ == bad) throw Error("graph failed"); }); } catch (const Error&) { thrown = true; }
      CHECK(thrown && n == bad + 1 && !A.dry && g_ensures == bad);
    }
    // the handle works after a failed call
    int n = 0;
    arena_passes(A, [&] { ++n; });
    CHECK(n == 2 && !A.dry);
  }
  {  // ZeroedBlock: the decision alone (stale / remember); ensure_zero adds the memset on a real pass
    ZeroedBlock Z;
    char blk[2];
    int clears = 0;
    auto offer = [&](const void* b, unsigned g, size_t n, int k0, int k1) { const bool c = Z.stale(b, g, n, k0, k1); if (c) { ++clears; Z.remember(b, g, n, k0, k1); } return c; };
    CHECK(offer(blk, 1, 4096, 50, 30));          // first use
    CHECK(!offer(blk, 1, 4096, 50, 30));         // the same block again
    CHECK(offer(blk + 1, 1, 4096, 50, 30));      // base
    CHECK(offer(blk + 1, 2, 4096, 50, 30));      // arena generation
    CHECK(offer(blk + 1, 2, 8192, 50, 30));      // bytes
    CHECK(offer(blk + 1, 2, 8192, 51, 30));      // first key
    CHECK(offer(blk + 1, 2, 8192, 51, 31));      // second key
    CHECK(!offer(blk + 1, 2, 8192, 51, 31));
    Z.reset();
    CHECK(offer(blk + 1, 2, 8192, 51, 31));      // after reset()
    CHECK(!offer(blk + 1, 2, 8192, 51, 31) && clears == 7);
    ZeroedBlock fresh;
    CHECK(fresh.stale(nullptr, 0, 0, 0, 0) && fresh.stale(blk, 0, 0, -1, -1));   // a default block matches no keyed layout and no real base
    ZeroedBlock copy = Z; Z = {};
    CHECK(Z.stale(blk + 1, 2, 8192, 51, 31) && !copy.stale(blk + 1, 2, 8192, 51, 31));   // `= {}` over a model's weights forgets the block
  }
  return 0;
}
