// aej_spans.h -- the span check of the packed-image entries (aej_filter_batch, aej_window_batch, aej_resample_batch*, aej_warp_batch,
// aej_adjust_batch / aej_histogram_batch, aej_compose_batch): what a call reads and writes, as byte spans, and the one rule they are held
// to.  Plain host C++, nothing of HIP: tests/native/spans_check.cpp compiles it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace aej {

// bytes [offset, offset + bytes) of the source buffer that an image's kernels read, or elements [offset, offset + bytes) of the output
// that they write (`bytes` counts the output's own elements there: bytes but for aej_histogram_batch's int64)
struct Span { int image; long long offset, bytes; };

// what a plan says about the call's memory: the reads image by image, every read of an image together (compose has up to three), and
// one write per image, in the same order
struct Spans { std::vector<Span> reads, writes; };

enum SpanFault { kSpanFine = 0, kSpanSourceOutside, kSpanImageOutside, kSpanSourceInside };
struct SpanVerdict { SpanFault fault; int image; };

// The first fault of a call, image by image: that image's sources outside [0, src_bytes) of the input, then its image outside
// [0, dst_elements) of the output, then its sources meeting the output's dst_elements * dst_unit bytes.  Every range is half-open: a
// source that ends where the output begins, or begins where it ends, is fine.
// (src_bytes may span memory between separate images, the output among it: what must not meet the output is each image's source.)
inline SpanVerdict span_fault(const Spans &s, uintptr_t src, uint64_t src_bytes, uintptr_t dst, uint64_t dst_elements, uint64_t dst_unit)
{
    const uintptr_t dst_end = dst + (uintptr_t)(dst_elements * dst_unit);
    size_t r = 0;
    for (const Span &w : s.writes) {
        const size_t first = r;
        while (r < s.reads.size() && s.reads[r].image == w.image) r++;
        for (size_t k = first; k < r; k++)
            if ((uint64_t)s.reads[k].offset + (uint64_t)s.reads[k].bytes > src_bytes) return { kSpanSourceOutside, w.image };
        if ((uint64_t)w.offset + (uint64_t)w.bytes > dst_elements) return { kSpanImageOutside, w.image };
        for (size_t k = first; k < r; k++) {
            const uintptr_t a = src + (uintptr_t)s.reads[k].offset;
            if (a < dst_end && dst < a + (uintptr_t)s.reads[k].bytes) return { kSpanSourceInside, w.image };
        }
    }
    return { kSpanFine, -1 };
}

}  // namespace aej
