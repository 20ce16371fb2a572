// spans_check.cpp -- prints what aej::span_fault (csrc/aej_spans.h, the span check of the packed-image entries) answers for a list of
// calls, one line each: "name | src src_bytes dst dst_elements dst_unit | reads | writes -> fault image", a span as image:offset:bytes.
// tests/test_spans_host.py compiles this with the host compiler, checks every line against the rule worked out again in Python and the
// named cases against their answers.  Nothing of HIP and no device.
#include <stdio.h>

#include "../../adaptive_edge_aware_jpeg_amd/csrc/aej_spans.h"

using aej::Span;
using aej::Spans;

static void row(const char *name, uintptr_t src, uint64_t src_bytes, uintptr_t dst, uint64_t dst_elements, uint64_t unit, const Spans &s)
{
    const aej::SpanVerdict v = aej::span_fault(s, src, src_bytes, dst, dst_elements, unit);
    printf("%s | %llu %llu %llu %llu %llu |", name, (unsigned long long)src, (unsigned long long)src_bytes, (unsigned long long)dst,
           (unsigned long long)dst_elements, (unsigned long long)unit);
    for (const Span &r : s.reads) printf(" %d:%lld:%lld", r.image, r.offset, r.bytes);
    printf(" |");
    for (const Span &w : s.writes) printf(" %d:%lld:%lld", w.image, w.offset, w.bytes);
    printf(" -> %d %d\n", (int)v.fault, v.image);
}

int main()
{
    const uintptr_t S = 1000, D = 2000;
    const Spans one = { { { 0, 0, 12 } }, { { 0, 0, 12 } } };      // one image: a 12-byte source at the input's start, a 12-byte output
    // ---- the edges of the input and of the output
    row("source ends at src_bytes", S, 12, D, 12, 1, one);
    row("source one byte past src_bytes", S, 11, D, 12, 1, one);
    row("image ends at the output's end", S, 12, D, 12, 1, one);
    row("image one element past the output", S, 12, D, 11, 1, one);
    // ---- the source against the output
    row("source ends at the output's first byte", S, 12, S + 12, 12, 1, one);
    row("source begins after the output's last byte", S, 12, S - 12, 12, 1, one);
    row("one byte of overlap, the source below", S, 12, S + 11, 12, 1, one);
    row("one byte of overlap, the source above", S, 12, S - 11, 12, 1, one);
    row("source wholly inside a larger output", S, 12, S - 10, 40, 1, one);
    const Spans apart = { { { 0, 0, 12 }, { 1, 100, 12 } }, { { 0, 0, 12 }, { 1, 12, 12 } } };
    row("output inside the source span, meeting no image", S, 112, S + 40, 24, 1, apart);
    // ---- an output of two 8-byte elements: the bounds count elements, the overlap bytes
    const Spans wide = { { { 0, 0, 12 } }, { { 0, 0, 2 } } };
    row("8-byte elements, source at the output + 2", D + 2, 12, D, 2, 8, wide);
    row("8-byte elements, source at the output + 15", D + 15, 12, D, 2, 8, wide);
    row("8-byte elements, source at the output + 16", D + 16, 12, D, 2, 8, wide);
    row("8-byte elements, source ends at the output", D - 12, 12, D, 2, 8, wide);
    row("8-byte elements, source ends one byte inside", D - 11, 12, D, 2, 8, wide);
    row("8-byte elements, third element", S, 12, D, 2, 8, Spans{ { { 0, 0, 12 } }, { { 0, 1, 2 } } });
    // ---- which fault is reported
    row("image 0 outside the output, image 1 outside the input", S, 24, D, 24, 1, Spans{ { { 0, 0, 12 }, { 1, 13, 12 } }, { { 0, 13, 12 }, { 1, 0, 12 } } });
    row("image 0 inside the output, image 1 outside the input", S, 24, S + 4, 24, 1, Spans{ { { 0, 0, 12 }, { 1, 13, 12 } }, { { 0, 0, 12 }, { 1, 12, 12 } } });
    row("image 0 fine, image 1 outside the output", S, 24, D, 23, 1, Spans{ { { 0, 0, 12 }, { 1, 12, 12 } }, { { 0, 0, 12 }, { 1, 12, 12 } } });
    row("outside the input and outside the output", S, 11, D, 11, 1, one);
    row("outside the output and inside it", S, 12, S + 4, 11, 1, one);
    row("outside the input and inside the output", S, 11, S + 4, 12, 1, one);
    // ---- several reads of one image (compose: base, overlay, mask)
    const Spans three = { { { 0, 0, 12 }, { 0, 12, 6 }, { 0, 18, 4 } }, { { 0, 0, 12 } } };
    row("three reads, all fine", S, 22, D, 12, 1, three);
    row("three reads, the last outside the input", S, 21, D, 12, 1, three);
    row("three reads, the second outside the input", S, 17, D, 12, 1, Spans{ { { 0, 0, 12 }, { 0, 12, 6 }, { 0, 0, 4 } }, { { 0, 0, 12 } } });
    row("three reads, the last inside the output", S, 22, S + 21, 12, 1, three);
    row("three reads, the first inside the output", S, 22, S - 11, 12, 1, three);
    row("two images of two reads, image 1's second outside", S, 40, D, 24, 1,
        Spans{ { { 0, 0, 12 }, { 0, 12, 6 }, { 1, 18, 12 }, { 1, 30, 11 } }, { { 0, 0, 12 }, { 1, 12, 12 } } });
    row("image 0's second read inside, image 1's first outside", S, 40, S + 17, 24, 1,
        Spans{ { { 0, 0, 12 }, { 0, 12, 6 }, { 1, 30, 12 } }, { { 0, 0, 12 }, { 1, 12, 12 } } });
    // ---- every place of a 12-byte source about a 12-byte output, and every size of either buffer about 12
    for (int at = -14; at <= 14; at++) row("sweep: the source about the output", D + at, 12, D, 12, 1, one);
    for (int size = 10; size <= 14; size++) {
        row("sweep: src_bytes", S, size, D, 12, 1, one);
        row("sweep: dst_elements", S, 12, D, size, 1, one);
    }
    return 0;
}
