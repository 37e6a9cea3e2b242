// The one-allocation table of a module's setter, laid out in one place.  A setter declares its sections -- doubles,
// int32 tables, byte tables -- in any order; the image puts every double section first (8-byte aligned), then the
// int32 sections, packed, then the byte sections from the next 8-byte boundary, and rounds the whole up to 8 bytes.
// A section's handle becomes a typed pointer against any base that holds the image: the host copy here, or the device
// allocation it was uploaded to.  A section of zero elements is legal and takes no space; its pointer is that of
// whatever follows and must not be dereferenced.  Host only, no HIP: a plain C++ compiler builds it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ms {

class TableBlob {
 public:
  // a section's place among the sections of its kind, in elements
  struct F64 { size_t at; };
  struct I32 { size_t at; };
  struct U8 { size_t at; };

  // n elements, zero-filled or copied from src (n of them); every f64 / i32 / u8 call comes before image()
  F64 f64(size_t n, const double* src = nullptr) { return {grow(f64_, n, src)}; }
  I32 i32(size_t n, const int32_t* src = nullptr) { return {grow(i32_, n, src)}; }
  U8 u8(size_t n, const uint8_t* src = nullptr) { return {grow(u8_, n, src)}; }
  I32 i32(const std::vector<int32_t>& v) { return i32(v.size(), v.data()); }

  // bytes of the image; never 0 (a setter's allocation is also what says its table is set)
  size_t bytes() const { return std::max<size_t>(8, round8(u8_begin() + u8_.size())); }

  // the host image: the sections in place, every other byte zero.  Valid until the next section is declared.
  void* image() {
    img_.assign(bytes() / 8, 0.0);
    put(at(img_.data(), F64{0}), f64_);
    put(at(img_.data(), I32{0}), i32_);
    put(at(img_.data(), U8{0}), u8_);
    return img_.data();
  }

  // a section inside the image that starts at base
  double* at(void* base, F64 h) const { return static_cast<double*>(base) + h.at; }
  int32_t* at(void* base, I32 h) const { return reinterpret_cast<int32_t*>(static_cast<double*>(base) + f64_.size()) + h.at; }
  uint8_t* at(void* base, U8 h) const { return static_cast<uint8_t*>(base) + u8_begin() + h.at; }
  // (a kernel's arrival counter lives in a double's cell)
  uint32_t* u32(void* base, F64 h) const { return reinterpret_cast<uint32_t*>(at(base, h)); }

 private:
  static size_t round8(size_t n) { return (n + 7) / 8 * 8; }
  size_t u8_begin() const { return round8(sizeof(double) * f64_.size() + sizeof(int32_t) * i32_.size()); }
  template <class T>
  static size_t grow(std::vector<T>& v, size_t n, const T* src) {
    const size_t o = v.size();
    if (src && n) v.insert(v.end(), src, src + n);
    else v.resize(o + n, T(0));
    return o;
  }
  template <class T>
  static void put(T* dst, const std::vector<T>& v) {
    if (!v.empty()) memcpy(dst, v.data(), sizeof(T) * v.size());
  }
  std::vector<double> f64_, img_;
  std::vector<int32_t> i32_;
  std::vector<uint8_t> u8_;
};

}  // namespace ms
