// The layout of csrc/ms_table_blob.h, checked on the host: built with -fsanitize=address,undefined and run by
// tests/test_table_blob_host.py.  For each shape: the sections lie inside the image and do not overlap, doubles are
// 8-byte and ints 4-byte aligned, given sources are copied in, every other byte is zero, and writing every element of
// every section through the resolved pointers -- against a copy of the image of exactly bytes() bytes, as the device
// allocation is -- stays inside it (the sanitizer is the judge of that).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ms_table_blob.h"

using ms::TableBlob;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAIL %s: %s -- ", name, #cond);        \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      ++g_failed;                                         \
    }                                                     \
  } while (0)

struct Shape {
  const char* name;
  TableBlob b;
  struct Sec {
    char kind;  // 'd', 'i', 'b'
    size_t n;
    bool sourced;
    TableBlob::F64 d;
    TableBlob::I32 i;
    TableBlob::U8 u;
  };
  std::vector<Sec> secs;
  int salt = 1;

  explicit Shape(const char* nm) : name(nm) {}
  // a section of n elements; sourced: filled from a non-zero pattern of its own, else left to the builder's zeros
  void f64(size_t n, bool sourced = false) {
    std::vector<double> src(n);
    for (size_t k = 0; k < n; ++k) src[k] = 1000.0 * salt + (double)k + 0.5;
    secs.push_back({'d', n, sourced, b.f64(n, sourced ? src.data() : nullptr), {0}, {0}});
    ++salt;
  }
  void i32(size_t n, bool sourced = false) {
    std::vector<int32_t> src(n);
    for (size_t k = 0; k < n; ++k) src[k] = (int32_t)(1000 * salt + (int)k + 1);
    secs.push_back({'i', n, sourced, {0}, b.i32(n, sourced ? src.data() : nullptr), {0}});
    ++salt;
  }
  void u8(size_t n, bool sourced = false) {
    std::vector<uint8_t> src(n);
    for (size_t k = 0; k < n; ++k) src[k] = (uint8_t)(1 + (salt + k) % 255);
    secs.push_back({'b', n, sourced, {0}, {0}, b.u8(n, sourced ? src.data() : nullptr)});
    ++salt;
  }

  static size_t elem(const Sec& s) { return s.kind == 'd' ? 8 : s.kind == 'i' ? 4 : 1; }
  uint8_t* ptr(void* base, const Sec& s) const {
    return s.kind == 'd'   ? reinterpret_cast<uint8_t*>(b.at(base, s.d))
           : s.kind == 'i' ? reinterpret_cast<uint8_t*>(b.at(base, s.i))
                           : b.at(base, s.u);
  }

  void check() {
    const size_t total = b.bytes();
    uint8_t* img = static_cast<uint8_t*>(b.image());
    CHECK(total >= 8 && total % 8 == 0, "total %zu", total);
    CHECK(reinterpret_cast<uintptr_t>(img) % 8 == 0, "the image itself is not 8-byte aligned");
    std::vector<int> owner(total, -1);  // which section holds each byte
    int salt_k = 1;
    for (size_t k = 0; k < secs.size(); ++k, ++salt_k) {
      const Sec& s = secs[k];
      const size_t lo = (size_t)(ptr(img, s) - img), hi = lo + s.n * elem(s);
      CHECK(lo <= total && hi <= total, "section %zu spans [%zu, %zu) of %zu", k, lo, hi, total);
      if (hi > total) return;
      if (s.n > 0) {
        const size_t want = s.kind == 'b' ? 1 : elem(s);
        CHECK(lo % want == 0, "section %zu (%c) starts at byte %zu", k, s.kind, lo);
      }
      for (size_t q = lo; q < hi; ++q) {
        CHECK(owner[q] < 0, "byte %zu belongs to sections %d and %zu", q, owner[q], k);
        owner[q] = (int)k;
      }
      // the source, or zeros
      for (size_t e = 0; e < s.n; ++e) {
        if (s.kind == 'd') {
          double v;
          std::memcpy(&v, img + lo + 8 * e, 8);
          CHECK(v == (s.sourced ? 1000.0 * salt_k + (double)e + 0.5 : 0.0), "section %zu element %zu holds %g", k, e, v);
        } else if (s.kind == 'i') {
          int32_t v;
          std::memcpy(&v, img + lo + 4 * e, 4);
          CHECK(v == (s.sourced ? (int32_t)(1000 * salt_k + (int)e + 1) : 0), "section %zu element %zu holds %d", k, e, v);
        } else {
          const uint8_t v = img[lo + e];
          CHECK(v == (s.sourced ? (uint8_t)(1 + (salt_k + e) % 255) : 0), "section %zu element %zu holds %u", k, e, v);
        }
      }
    }
    for (size_t q = 0; q < total; ++q)
      if (owner[q] < 0) CHECK(img[q] == 0, "padding byte %zu holds %u", q, img[q]);
    // the kinds in the image's order: every double before every int before every byte
    size_t d_hi = 0, i_lo = total, i_hi = 0, b_lo = total;
    for (const Sec& s : secs) {
      if (s.n == 0) continue;
      const size_t lo = (size_t)(ptr(img, s) - img), hi = lo + s.n * elem(s);
      if (s.kind == 'd') d_hi = std::max(d_hi, hi);
      if (s.kind == 'i') i_lo = std::min(i_lo, lo), i_hi = std::max(i_hi, hi);
      if (s.kind == 'b') b_lo = std::min(b_lo, lo);
    }
    CHECK(d_hi <= i_lo && d_hi <= b_lo && i_hi <= b_lo, "kinds out of order: doubles end %zu, ints [%zu, %zu), bytes from %zu",
          d_hi, i_lo, i_hi, b_lo);
    // the same handles against another base of exactly `total` bytes: every element written, then read back
    uint8_t* dev = static_cast<uint8_t*>(std::malloc(total));
    std::memcpy(dev, img, total);
    for (const Sec& s : secs) {
      CHECK(ptr(dev, s) - dev == ptr(img, s) - img, "a handle resolves differently against another base");
      for (size_t e = 0; e < s.n; ++e) {
        if (s.kind == 'd') b.at(dev, s.d)[e] = -1.0 - (double)e;
        if (s.kind == 'i') b.at(dev, s.i)[e] = -1 - (int32_t)e;
        if (s.kind == 'b') b.at(dev, s.u)[e] = (uint8_t)(255 - e % 200);
      }
    }
    for (const Sec& s : secs)
      for (size_t e = 0; e < s.n; ++e) {
        if (s.kind == 'd') CHECK(b.at(dev, s.d)[e] == -1.0 - (double)e, "a later write reached a double section");
        if (s.kind == 'i') CHECK(b.at(dev, s.i)[e] == -1 - (int32_t)e, "a later write reached an int section");
        if (s.kind == 'b') CHECK(b.at(dev, s.u)[e] == (uint8_t)(255 - e % 200), "a later write reached a byte section");
      }
    for (size_t q = 0; q < total; ++q)
      if (owner[q] < 0) CHECK(dev[q] == 0, "a section's write reached padding byte %zu", q);
    std::free(dev);
    std::printf("ok %s: %zu sections, %zu bytes\n", name, secs.size(), total);
  }
};

// ms_set_thetab_boundary's table for a ring of n rows with two facets a row: d, N_v; rows, off, fv; keep
void thetab_boundary(size_t n) {
  static char names[3][40];
  static int used = 0;
  std::snprintf(names[used], sizeof(names[used]), "thetab_boundary n=%zu", n);
  Shape s(names[used++]);
  s.f64(3 * n);
  s.f64(3 * n);
  s.i32(n, true);
  s.i32(n + 1, true);
  s.i32(6 * n, true);  // (n + n + 1 + 6 n ints: an odd count)
  s.u8(n);             // (1, 3, 9 bytes: no multiple of 8)
  s.check();
}

}  // namespace

int main() {
  {
    Shape s("no section");
    s.check();
  }
  {
    Shape s("every section empty");
    s.f64(0);
    s.i32(0, true);
    s.u8(0);
    s.f64(0, true);
    s.check();
  }
  {
    Shape s("one double and one int");
    s.f64(1, true);
    s.i32(1, true);
    s.check();
  }
  {
    Shape s("sections declared out of the image's order");
    s.u8(5, true);
    s.i32(3, true);
    s.f64(2, true);
    s.u8(0);
    s.i32(0);
    s.f64(1);
    s.check();
  }
  thetab_boundary(1);
  thetab_boundary(3);
  thetab_boundary(9);
  {
    // ms_set_rim_match's table with n_rim = 1, n_outer = 2, n_disk = 0 (one slot in each of the disk's tables)
    const size_t nr = 1, no = 2, nd = 1;
    Shape s("rim_slope_match n_rim=1 n_outer=2 n_disk=0");
    s.f64(3 * nr);
    for (int k = 0; k < 7; ++k) s.f64(nr);
    s.f64(no);
    s.f64(3 * nd);
    s.f64(nd);
    s.f64(6);
    s.f64(1);
    s.f64(1);
    s.f64(1);
    s.i32(nr, true);
    s.i32(no, true);
    s.i32(nd, true);
    s.i32(nr, true);
    s.i32(no, true);
    s.i32(nd, true);
    s.i32(nr);
    s.i32(nr);
    s.i32(no + 1);
    s.check();
  }
  if (g_failed) {
    std::printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("all shapes ok\n");
  return 0;
}
