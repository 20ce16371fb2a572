// aej_sched.h -- the arithmetic of the stream-priority policy (aej_set_option "stream_priorities"): plain C++, no HIP, so that a host
// test can compile it alone (tests/test_stream_priorities_host.py).
//
// The HIP runtime keeps its pool of reusable hardware queues per stream priority and compares GPU_MAX_HW_QUEUES with the size of the
// pool of the priority asked for: streams of another priority get queues from a pool of their own.  A process whose runtime started
// with few queues can therefore still give its sub-batch streams queues of their own, by creating them with priorities.
#pragma once

namespace aej {

constexpr int kMaxProcessQueues = 32;      // hardware queues a process may hold in all
constexpr int kWideScheduleQueues = 8;     // from this many queues on every part stream has a queue of its own (sub_batches() of api_encode.hip)

// priority levels by the index the policy deals (api_encode.hip maps them onto hipDeviceGetStreamPriorityRange)
enum PriorityLevel { kPrioNormal = 0, kPrioHigh = 1, kPrioLow = 2 };

// "stream_priority_pattern": which levels the part streams of a process are dealt, in creation order
//   0 normal, high, normal, ...   1 normal, low, normal, ...   2 normal, high, low, normal, ...   3 high, low, high, ...
// 3 is the default: the measured best (profiles/stream_priorities_ab.txt); a part at the normal level beside parts at another ran
// slower than no priorities at all.
constexpr int kPriorityPatterns = 4;
constexpr int kDefaultPriorityPattern = 3;
inline int priority_levels(int pattern) { return pattern == 2 ? 3 : 2; }
inline int priority_level_of(int pattern, unsigned long long k)      // of the k-th part stream the process creates with a priority
{
    switch (pattern) {
    case 0: return k & 1 ? kPrioHigh : kPrioNormal;
    case 1: return k & 1 ? kPrioLow : kPrioNormal;
    case 2: return k % 3 == 0 ? kPrioNormal : k % 3 == 1 ? kPrioHigh : kPrioLow;
    default: return k & 1 ? kPrioLow : kPrioHigh;
    }
}

// mode ("stream_priorities"): 0 never, 1 automatic (only when the process has fewer queues than the wide schedule wants), 2 always
inline bool priorities_in_use(int mode, int hw_queues) { return mode == 2 || (mode == 1 && hw_queues < kWideScheduleQueues); }

// queues the part streams can spread over: one pool per level in use
inline int effective_hw_queues(int mode, int pattern, int hw_queues)
{
    return priorities_in_use(mode, hw_queues) ? hw_queues * priority_levels(pattern) : hw_queues;
}

// Only "always" can ask for more queues than a process may hold: the automatic mode stops at 7 queues x 3 levels = 21.
inline bool priorities_refused(int mode, int pattern, int hw_queues)
{
    return mode == 2 && (long long)hw_queues * priority_levels(pattern) > kMaxProcessQueues;
}

}  // namespace aej
