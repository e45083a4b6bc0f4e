// fpx_host_res.hpp -- the owners of the engine's host-side HIP resources (no device code).
//
// A buffer or an event that outlives a statement has an owner: one of the types below (none can be copied), as a member of the
// engine (what lives between calls) or as a local variable (what lives for one call; every return path frees it).
//   Scratch            a grow-only device buffer, or its pinned-host twin
//   Events<N>          N events created together
//   IntervalTimer<N>   the per-step event sets of one timer and the times they add up to
//   RankSum            the sums over the ranks of one output accumulator: receive buffer, extent, validity
//   FileCloser         a FILE * that is closed on every return path (the files the engine reads, and the checkpoint;
//                      every other file it writes has its owner in fpx_recfile.hpp)
// The buffers that live as long as the engine itself stay in its `owned` list (Engine::dalloc).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <initializer_list>
#include <utility>
#include <vector>

namespace fpx {

class Scratch {
  void *p_ = nullptr;
  size_t bytes_ = 0;
  bool pinned_;
  void drop() {
    if (p_) (void)(pinned_ ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr; bytes_ = 0;
  }

 public:
  explicit Scratch(bool pinned = false) : pinned_(pinned) {}
  Scratch(Scratch &&o) noexcept : p_(o.p_), bytes_(o.bytes_), pinned_(o.pinned_) { o.p_ = nullptr; o.bytes_ = 0; }
  Scratch &operator=(Scratch &&o) noexcept {
    if (this != &o) { drop(); p_ = o.p_; bytes_ = o.bytes_; pinned_ = o.pinned_; o.p_ = nullptr; o.bytes_ = 0; }
    return *this;
  }
  ~Scratch() { drop(); }

  // At least `bytes` and at least 16 afterwards, so the pointer is never null after a success (rocprim reads a null
  // temporary as a size query).  Growing waits for the work on `stream` that may still use the old buffer and does not
  // keep its contents; a failed allocation leaves the object empty.
  hipError_t reserve(size_t bytes, hipStream_t stream) {
    if (p_ && bytes <= bytes_) return hipSuccess;
    hipError_t e = release(stream);
    if (e != hipSuccess) return e;
    bytes = std::max<size_t>(bytes, 16);
    e = pinned_ ? hipHostMalloc(&p_, bytes) : hipMalloc(&p_, bytes);
    if (e != hipSuccess) { p_ = nullptr; return e; }
    bytes_ = bytes;
    return hipSuccess;
  }
  hipError_t release(hipStream_t stream) {
    if (!p_) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(stream);
    drop();
    return e;
  }
  size_t bytes() const { return bytes_; }
  template <typename T = void>
  T *as() const { return (T *)p_; }
};

template <int N>
class Events {
  hipEvent_t e_[N] = {};

 public:
  Events() = default;
  Events(Events &&o) noexcept { for (int i = 0; i < N; i++) { e_[i] = o.e_[i]; o.e_[i] = nullptr; } }
  Events &operator=(Events &&) = delete;
  ~Events() { for (int i = 0; i < N; i++) if (e_[i]) (void)hipEventDestroy(e_[i]); }
  hipError_t create() {
    for (int i = 0; i < N; i++) {
      const hipError_t e = hipEventCreate(&e_[i]);
      if (e != hipSuccess) { e_[i] = nullptr; return e; }
    }
    return hipSuccess;
  }
  hipEvent_t operator[](int i) const { return e_[i]; }
};

// One set of N events per step and the elapsed times between the pairs of them declared at construction, summed over the
// steps.  A step takes a set with begin(), records its events on the stream and calls commit() once the last of them is
// in the stream: only a committed set is ever read, so a step that fails half-way leaves nothing behind.  The sets are
// reused after a harvest; begin() harvests by itself once 64 are waiting, which bounds the pool in runs that never ask.
template <int N>
class IntervalTimer {
  std::vector<std::pair<int, int>> iv_;
  std::vector<double> acc_;
  std::vector<Events<N>> sets_;
  size_t used_ = 0;
  long long launches_ = 0;

 public:
  IntervalTimer(std::initializer_list<std::pair<int, int>> intervals) : iv_(intervals), acc_(intervals.size(), 0.) {}
  hipError_t begin(hipStream_t stream) {
    if (used_ >= 64) { const hipError_t e = harvest(stream); if (e != hipSuccess) return e; }
    if (used_ == sets_.size()) {
      Events<N> s;
      const hipError_t e = s.create();
      if (e != hipSuccess) return e;
      sets_.push_back(std::move(s));
    }
    return hipSuccess;
  }
  const Events<N> &current() const { return sets_[used_]; }   // the set of the last begin(); stays valid past commit()
  void commit() { used_++; }
  hipError_t harvest(hipStream_t stream) {
    const size_t n = used_;
    used_ = 0;                                     // whatever happens below, no set is read twice
    hipError_t e = hipStreamSynchronize(stream);
    for (size_t i = 0; i < n && e == hipSuccess; i++) {
      for (size_t k = 0; k < iv_.size() && e == hipSuccess; k++) {
        float t = 0;
        e = hipEventElapsedTime(&t, sets_[i][iv_[k].first], sets_[i][iv_[k].second]);
        if (e == hipSuccess) acc_[k] += t;
      }
      if (e == hipSuccess) launches_++;
    }
    return e;
  }
  // ms: one sum per declared interval
  hipError_t read(hipStream_t stream, double *ms, long long *launches, bool reset) {
    const hipError_t e = harvest(stream);
    if (e != hipSuccess) return e;
    for (size_t k = 0; k < iv_.size(); k++) ms[k] = acc_[k];
    if (launches) *launches = launches_;
    if (reset) { std::fill(acc_.begin(), acc_.end(), 0.); launches_ = 0; }
    return hipSuccess;
  }
};

// What goes with one output accumulator (gridunc, drygridunc, ..., flux, init_cond) once several ranks share a run: the
// receive buffer of its reduction (the reference's gridunc0, drygridunc0, ...: mpi_mod.f90:2451-2492,2543-2569), allocated
// with the first reduction, the accumulator's extent, and whether the buffer holds the sums of the partial sums as they
// are now.  The partial sums themselves stay where the kernels read them.  Who reduces, who reads and what makes the
// sums stale is the engine's business (Engine::reduce, source, and the invalidate() calls next to the kernels' launches).
class RankSum {
  void *recv_ = nullptr;
  size_t n_ = 0, elem_ = 0;
  bool valid_ = false;

 public:
  RankSum() = default;
  RankSum(const RankSum &) = delete;
  RankSum &operator=(const RankSum &) = delete;
  ~RankSum() { if (recv_) (void)hipFree(recv_); }
  void shape(size_t count, size_t elem_bytes) { n_ = count; elem_ = elem_bytes; }   // once, when the accumulator is allocated
  size_t count() const { return n_; }
  size_t elem() const { return elem_; }       // 4 or 8: the element is a float or a double
  size_t bytes() const { return n_ * elem_; }
  hipError_t reserve() { return recv_ ? hipSuccess : hipMalloc(&recv_, std::max<size_t>(bytes(), 1)); }
  void *recv() const { return recv_; }
  bool valid() const { return valid_; }
  void filled() { valid_ = true; }
  void invalidate() { valid_ = false; }
};

struct FileCloser {
  FILE *f;
  explicit FileCloser(FILE *file) : f(file) {}
  FileCloser(const FileCloser &) = delete;
  FileCloser &operator=(const FileCloser &) = delete;
  ~FileCloser() { if (f) fclose(f); }
  int close() { FILE *g = f; f = nullptr; return g ? fclose(g) : 0; }   // fclose's result, for the writers that check it
};

}  // namespace fpx
