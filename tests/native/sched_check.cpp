// Prints the stream-priority policy of csrc/aej_sched.h (the header the library compiles) as a table for
// tests/test_stream_priorities_host.py:  mode pattern hw_queues -> in_use levels effective refused dealt(12 levels, in creation order)
#include <stdio.h>

#include "../../adaptive_edge_aware_jpeg_amd/csrc/aej_sched.h"

int main()
{
    printf("limits %d %d %d\n", aej::kMaxProcessQueues, aej::kWideScheduleQueues, aej::kPriorityPatterns);
    for (int mode = 0; mode <= 2; mode++)
        for (int pattern = 0; pattern < aej::kPriorityPatterns; pattern++)
            for (int q = 1; q <= 40; q++) {
                printf("%d %d %d -> %d %d %d %d ", mode, pattern, q, aej::priorities_in_use(mode, q) ? 1 : 0, aej::priority_levels(pattern),
                       aej::effective_hw_queues(mode, pattern, q), aej::priorities_refused(mode, pattern, q) ? 1 : 0);
                for (unsigned long long k = 0; k < 12; k++) printf("%d", aej::priority_level_of(pattern, k));
                printf("\n");
            }
    return 0;
}
