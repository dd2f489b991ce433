// fe_store_policy.h -- part of fe_env.hip: the per-launch store policy of a large single-asset observation, as a pure
// host function of (what the env remembers, the buffer this launch writes, its size).  Standard C++ only, no HIP
// include: tests/test_store_policy_host.py compiles it with the system compiler and drives it with pointer sequences.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>

// An observation buffer in this size class is singled out: two of them overflow the 256 MiB Infinity Cache
// (>= kFeObsStreamMinBytes), one of them fits it (<= kFeObsResidentMaxBytes).
constexpr uint64_t kFeObsStreamMinBytes = 128ull << 20;
constexpr uint64_t kFeObsResidentMaxBytes = 256ull << 20;
// Consecutive launches that have not written the resident buffer before the current one takes its place: more than any
// observation ring the project uses (2 or 3 members).
constexpr int kFeObsResidentPatience = 8;

// What an env remembers between launches.  Relaxed atomics: concurrent calls on different streams must not race, and a
// stale value costs one launch the other policy, never correctness.
struct FeObsResidency {
    std::atomic<const void *> resident{nullptr};  // the ONE buffer whose stores may stay in the Infinity Cache
    std::atomic<int> away{0};                     // consecutive launches that wrote some other buffer
};

// 1 = this launch streams its observation past the Infinity Cache (sc1 | nt), 0 = plain sc1.
//   * a buffer below the size class never streams, one above it always does; neither touches the state;
//   * a launch that writes the resident buffer stores plain -- the cache absorbs a buffer that is rewritten again and
//     again, also while other ring members stream past it;
//   * a launch that writes any other buffer streams, and when kFeObsResidentPatience consecutive launches have done so
//     (at once for an env that has no resident buffer yet) the buffer it writes becomes the resident one for the
//     launches after it.  Fresh tensors every call therefore stream every time, like before.
inline int fe_obs_store_policy(FeObsResidency &st, const void *obs, uint64_t bytes) {
    if (bytes < kFeObsStreamMinBytes) return 0;
    if (bytes > kFeObsResidentMaxBytes) return 1;
    const void *res = st.resident.load(std::memory_order_relaxed);
    if (res == obs) {
        st.away.store(0, std::memory_order_relaxed);
        return 0;
    }
    const int away = st.away.load(std::memory_order_relaxed) + 1;
    if (res == nullptr || away >= kFeObsResidentPatience) {
        st.resident.store(obs, std::memory_order_relaxed);
        st.away.store(0, std::memory_order_relaxed);
    } else {
        st.away.store(away, std::memory_order_relaxed);
    }
    return 1;
}
