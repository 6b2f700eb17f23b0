// lep_block.h -- the layout of a packed descriptor block, and the block itself: which arrays, at which offsets, copied from where.  Host
// code without a HIP call in it (lep_gpu.hip stages a Block through its pinned ring; tests/emu/stage_block_probe.cc walks it on the CPU).
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace lepbuf {

inline size_t round_up(size_t v, size_t align = 256) { return (v + align - 1) & ~(align - 1); }   // (align: a power of two)

// A packed block of arrays: add<T>(n) appends n elements at the next multiple of `align` and returns their offset; bytes() is where
// the last part ends, padded() that rounded up to 256.
struct Layout {
    size_t end = 0;
    template <class T> size_t add(size_t n, size_t align = 256) {
        const size_t off = round_up(end, align);
        end = off + n * sizeof(T);
        return off;
    }
    size_t bytes() const { return end; }
    size_t padded() const { return round_up(end); }
};

// A Layout that remembers where its parts come from.  add(src, n) is add<T>(n) -- the same offsets for the same calls -- and notes the
// host array the part is a copy of; a part added without one is the device's to fill (scratch, outputs, counters).  upload_bytes() is
// the end of the last part that has a source and an element, and pack() writes the image of [0, upload_bytes()): every such part at
// its offset, zero bytes in the gaps (and over a sourceless part in front of a sourced one: call sites keep the sourced parts in front).
struct Block : Layout {
    struct Part { size_t off; const void* src; size_t bytes; };
    std::vector<Part> parts;
    using Layout::add;
    template <class T> size_t add(const T* src, size_t n, size_t align = 256) {
        const size_t off = Layout::add<T>(n, align);
        if (n) parts.push_back(Part{off, src, n * sizeof(T)});
        return off;
    }
    size_t upload_bytes() const { return parts.empty() ? 0 : parts.back().off + parts.back().bytes; }
    void pack(char* dst) const {
        size_t at = 0;
        for (const Part& p : parts) {
            memset(dst + at, 0, p.off - at);
            memcpy(dst + p.off, p.src, p.bytes);
            at = p.off + p.bytes;
        }
    }
};

}  // namespace lepbuf
