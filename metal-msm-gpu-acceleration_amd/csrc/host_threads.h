// The thread split of the host twins (host_check.hip, host_compress.hip, host_mul.hip): items in T contiguous ranges.
#pragma once
#include <algorithm>
#include <thread>
#include <vector>

namespace msm_amd {

// threads <= 0: up to 16 host threads; never more threads than items, never none
inline unsigned worker_count(int threads, size_t items) {
  const unsigned want = threads > 0 ? (unsigned)threads : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  return (unsigned)std::max<size_t>(1, std::min<size_t>(want, items));
}

// fn(t, lo, hi) on T threads over [0, items): thread t takes the t-th range of ceil(items / T) items (the last ranges
// may be short or empty)
template <typename F>
void for_ranges(unsigned T, size_t items, F fn) {
  const size_t chunk = (items + T - 1) / T;
  auto worker = [&](unsigned t) {
    const size_t lo = std::min(items, t * chunk), hi = std::min(items, lo + chunk);
    fn(t, lo, hi);
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < T; ++t) pool.emplace_back(worker, t);
  worker(0);
  for (std::thread& th : pool) th.join();
}

}  // namespace msm_amd
