// fpx_recfile.hpp -- the owner of an output file and the one spelling of a Fortran unformatted sequential record (no HIP
// here: a plain host compiler builds it, tests/recfile_host.cpp).
//
// The files the engine writes are compared byte for byte with the reference's, whose records are: the payload's length
// in bytes as a 4-byte integer, the payload, the length again (the layout of the reference's compilers for records
// below 2 GiB; they split longer ones into subrecords, which nothing here writes).
//   RecFile            a FILE * that is closed on every return path, with a sticky error state
//     record(p, n)       one record from memory;  scalar(v): one record holding one value
//     put(...) / end()   one record assembled from several pieces
//     write(p, n)        bytes without markers (direct-access files, text, records a kernel has already framed)
//     close()            true if the open, every write and fclose itself succeeded
// After the first failure every further write is skipped; the caller asks once, at close().
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace fpx {

class RecFile {
  FILE *f_;
  bool ok_;
  std::vector<unsigned char> rec_;   // the record put() assembles

 public:
  static constexpr size_t kMaxRecord = 0x7fffffff;   // longer records would need subrecords
  explicit RecFile(const char *path, const char *mode = "wb") : f_(fopen(path, mode)), ok_(f_ != nullptr) {}
  RecFile(RecFile &&o) noexcept : f_(o.f_), ok_(o.ok_), rec_(std::move(o.rec_)) { o.f_ = nullptr; o.ok_ = false; }
  RecFile &operator=(RecFile &&) = delete;
  ~RecFile() { if (f_) fclose(f_); }

  bool is_open() const { return f_ != nullptr; }
  bool ok() const { return ok_; }
  void write(const void *p, size_t n) { ok_ = ok_ && (n == 0 || fwrite(p, 1, n, f_) == n); }
  void record(const void *p, size_t n) {
    ok_ = ok_ && n <= kMaxRecord;
    const int32_t len = (int32_t)n;
    write(&len, 4); write(p, n); write(&len, 4);
  }
  template <typename T>
  void scalar(const T &v) { record(&v, sizeof(T)); }
  void put(const void *p, size_t n) { const unsigned char *c = (const unsigned char *)p; rec_.insert(rec_.end(), c, c + n); }
  template <typename T>
  void put(const T &v) { put(&v, sizeof(T)); }
  void end() { record(rec_.data(), rec_.size()); rec_.clear(); }
  bool close() {
    if (f_) { ok_ = (fclose(f_) == 0) && ok_; f_ = nullptr; }
    return ok_;
  }
};

}  // namespace fpx
