// Host-only exercise of the device-memory owners of csrc/rvc_internal.h (DevBuf, OwnedConvLayer) over malloc / free: built with the host compiler and
// AddressSanitizer + UBSan by tests/test_dev_owners_host.py, no HIP runtime linked.  Exit status: the number of allocations still live at the end (0), or
// 100 when a check failed.
#include "rvc_internal.h"
#include <utility>

static long g_live = 0;
namespace rvc {
void set_error(const std::string&) {}
void* dev_alloc(size_t bytes) { ++g_live; return malloc(bytes ? bytes : 1); }
void* dev_upload(const void* host, size_t bytes) { void* d = dev_alloc(bytes); if (bytes) memcpy(d, host, bytes); return d; }
void dev_free(void* p) { if (p) { --g_live; free(p); } }
}  // namespace rvc
using namespace rvc;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(100); } } while (0)

static void fill(ConvLayer& L, int Co) {      // what the *_layer_init functions leave behind: all five weight allocations
  L.Wd_ = static_cast<float*>(dev_alloc(64)); L.bd_ = static_cast<float*>(dev_alloc(16)); L.bd4_ = static_cast<float*>(dev_alloc(16));
  L.Wx_ = static_cast<uint16_t*>(dev_alloc(32)); L.Wh_ = static_cast<uint16_t*>(dev_alloc(32));
  L.Co = Co;
}

struct Weights { OwnedConvLayer conv[3], proj; DevBuf<float> gamma; DevBuf<int> rows; std::vector<OwnedConvLayer> layers; int img_T = -1; bool pad_ok = false; };
struct Model : Weights { bool ready = false; };

int main() {
  {  // DevBuf: upload twice, reset, move-construct, move-assign, self-move-assign
    const std::vector<float> h = {1.f, 2.f, 3.f};
    DevBuf<float> a;
    a.upload(h); a.upload(h.data(), 2);
    CHECK(g_live == 1 && a.n == 2 && a.get()[1] == 2.f);
    a.reset();
    CHECK(g_live == 0 && !a.get() && a.n == 0);
    a.upload(h);
    DevBuf<float> b(std::move(a));
    CHECK(!a.p && a.n == 0 && b.n == 3 && g_live == 1);
    DevBuf<float> c; c.alloc(5);
    c = std::move(b);
    CHECK(g_live == 1 && !b.p && c.n == 3 && c.p[2] == 3.f);
    DevBuf<float>& alias = c;
    c = std::move(alias);
    CHECK(g_live == 1 && c.n == 3 && c.p[0] == 1.f);
    DevBuf<int> rows; rows.upload(std::vector<int>{4, 5});
    CHECK(rows.p[1] == 5 && g_live == 2);
  }
  CHECK(g_live == 0);
  {  // OwnedConvLayer in and out of a vector that grows past its capacity; a view dropped while its owner lives on
    std::vector<OwnedConvLayer> v;
    v.reserve(2);
    for (int i = 0; i < 5; ++i) { OwnedConvLayer L; fill(L, i); v.push_back(std::move(L)); CHECK(!L.Wd_ && !L.bd_ && !L.bd4_ && !L.Wx_ && !L.Wh_); }
    v.resize(9);
    CHECK(g_live == 25 && v[4].Co == 4 && v[4].Wh_ && !v[8].Wd_);
    OwnedConvLayer out = std::move(v[1]);
    CHECK(!v[1].Wd_ && !v[1].Wx_ && out.Co == 1 && out.bd4_);
    { ConvLayer view = out; view.Co = 7; CHECK(view.Wd_ == out.Wd_); }
    CHECK(g_live == 25 && out.Co == 1);
    v[0] = std::move(out);      // frees the five of v[0]
    CHECK(g_live == 20 && !out.Wd_ && v[0].Co == 1);
    v.resize(1);
    CHECK(g_live == 5);
  }
  CHECK(g_live == 0);
  {  // an aggregate of owners replaced by = {} (what *_finalize does with the model's weights)
    Model m;
    for (auto& c : m.conv) fill(c, 1);
    fill(m.proj, 2);
    m.gamma.upload(std::vector<float>(8, 1.f)); m.rows.alloc(3);
    m.layers.resize(4); for (auto& l : m.layers) fill(l, 3);
    m.img_T = 100; m.pad_ok = true; m.ready = true;
    CHECK(g_live == 5 * 8 + 2);
    static_cast<Weights&>(m) = {};
    CHECK(g_live == 0 && m.img_T == -1 && !m.pad_ok && m.layers.empty() && !m.conv[2].Wd_ && !m.gamma.p && m.ready);
    fill(m.conv[0], 1);
  }
  return (int)g_live;
}
