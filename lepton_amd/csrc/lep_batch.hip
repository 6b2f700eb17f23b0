// lep_batch.hip -- layer 3 of the C ABI for whole batches: `lepton in.jpg out.lep` / `lepton in.lep out.jpg` for many files
// at once, as a pipeline that keeps the GPU hot path fed (BASELINE.json configs[2-4]: hipStream-overlapped H2D / encode / D2H).
//
// Compression, chunk by chunk (two slots of staging buffers, chunk k+1 prepared while chunk k's coder kernels run):
//   host pool      split the files; the scans the GPU decoders take go up as scan bytes, the others are parsed here (jpeg_scan.cc)
//   scan stream    JPEG Huffman scan decode on the GPU straight into the device frames (lep_gpu_huffman_*decode*_device), row
//                  records down; the host pool finishes the hand-offs from them and parses again what the GPU refused
//   compute stream the coder kernels (lep_gpu_encode_device)
//                  [verify] the round trip on the GPU: decode what was just encoded into a scratch frame and compare frames
//                  (lep_compare_kernel); write the scans again from the frame and hold them against the file's own bytes
//                  (lep_scan_check_kernel, lep_scan_check_bytes_kernel) -- the reference's default `-verify`,
//                  src/lepton/validation.cc:97-218, costs it a second process and a full decode on the CPU
//   down stream    streams of chunk k come back, host pool writes the .lep containers (lep_container.cc) in the background
// Decompression is the mirror image: streams up, decoder kernels (lep_gpu_decode_device), then the JPEG Huffman scan encoders on the
// GPU (lep_gpu_huffman_encode_device, lep_gpu_huffman_progressive_encode_device) so that scan bytes come down instead of frames; the
// host pool glues headers and scans, and re-codes on the host only the files the GPU encoders do not take.
// Every size, offset and slot, and which stream a decompress launch takes, is lep_batch_layout.h's (host code, tested without a GPU);
// the stages below reserve, fill, upload and launch what it says.  The GPU work goes through the library's public entry points.
#include <hip/hip_runtime.h>
#include <malloc.h>
#include <sched.h>
#include <cstdio>

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <thread>
#include <vector>

#include "../../include/lepton_mi355x.h"
#include "jpeg_model.h"
#include "lep_batch_layout.h"
#include "lep_buffers.h"
#include "lep_container.h"
#include "lep_scan_routes.h"
static_assert(LEP_HUFFDEC_RST_TABLE == 2, "lep_scan_routes.h reads the flag by its value");
#include "lep_slice.h"

namespace {

std::atomic<uint64_t> g_scan_second_chances(0);   // lep_batch_scan_second_chances

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// CPUs this process may really use: affinity mask, capped by the cgroup CPU quota (a container can see 256 CPUs and be
// allowed 16: a pool sized by hardware_concurrency() then runs 3x slower than one sized by the quota)
int effective_cpus() {
    int n = (int)std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::max(1, std::min(n, CPU_COUNT(&set)));
    double quota = 0;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {   // cgroup v2: "<quota|max> <period>"
        char q[32]; long period = 0;
        if (fscanf(f, "%31s %ld", q, &period) == 2 && q[0] != 'm' && period > 0) quota = atof(q) / (double)period;
        fclose(f);
    } else {
        long q = -1, p = 0;
        if (FILE* a = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(a, "%ld", &q) != 1) q = -1; fclose(a); }
        if (FILE* b = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(b, "%ld", &p) != 1) p = 0; fclose(b); }
        if (q > 0 && p > 0) quota = (double)q / (double)p;
    }
    if (quota >= 1.0) n = std::min(n, (int)(quota + 0.5));
    return std::max(1, n);
}

// run fn(i) for i in [0, n) on `threads` host threads
void parallel_for(int n, int threads, const std::function<void(int)>& fn) {
    if (n <= 0) return;
    threads = std::max(1, std::min(threads, n));
    std::atomic<int> next(0);
    auto worker = [&]() { for (int i; (i = next.fetch_add(1)) < n;) fn(i); };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
}

// 16 bytes per lane, grid-stride: frames are compared at HBM speed (2 x bytes read, nothing written unless they differ)
__global__ void lep_compare_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b, size_t n16, uint32_t* flag, uint32_t value) {
    bool diff = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 x = a[i], y = b[i];
        diff |= (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
    }
    if (diff) atomicOr(flag, value);
}

// Round-trip check of progressive files: one workgroup per scan compares what the GPU scan encoder has just written
// with the file's own bytes of that scan (uploaded beside the un-stuffed copy the decoder read); any difference -- the
// length, a byte, an encoder that gave up (bit 31 of its length) -- sets bit 1 of the image's flag word.
using ScanCheck = lep_scan_check;                           // { out_off, ref_off, ref_len, image }: public for the test hooks
constexpr uint32_t kScanCheckPrefix = LEP_SCAN_CHECK_PREFIX;   // ScanCheck::image: the scan a file ends in -- written whole, its first ref_len bytes are the file's
__global__ void lep_scan_check_kernel(const uint8_t* __restrict__ out, const uint32_t* __restrict__ out_len, const uint8_t* __restrict__ ref,
                                      const ScanCheck* __restrict__ items, uint32_t* flags) {
    ScanCheck it = items[blockIdx.x];
    // (a prefix: what was written may well have outgrown a slot sized for the part the file kept; the bytes in front of that hold)
    bool diff = (it.image & kScanCheckPrefix) ? (out_len[blockIdx.x] & 0x7fffffffu) < it.ref_len : out_len[blockIdx.x] != it.ref_len;
    it.image &= ~kScanCheckPrefix;
    if (!diff) {
        const uint4* a = reinterpret_cast<const uint4*>(out + it.out_off);   // both 16-byte aligned
        const uint4* b = reinterpret_cast<const uint4*>(ref + it.ref_off);
        const uint32_t n16 = it.ref_len / 16;
        for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) {
            const uint4 x = a[i], y = b[i];
            diff |= (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
        }
        for (uint32_t i = n16 * 16 + threadIdx.x; i < it.ref_len; i += blockDim.x) diff |= out[it.out_off + i] != ref[it.ref_off + i];
    }
    if (diff) atomicOr(flags + it.image, 2u);
}

// the same against reference bytes at any alignment (a baseline file's thread segments, as they stand in the file)
__global__ void lep_scan_check_bytes_kernel(const uint8_t* __restrict__ out, const uint32_t* __restrict__ out_len, const uint8_t* __restrict__ ref,
                                            const ScanCheck* __restrict__ items, uint32_t* flags) {
    const ScanCheck it = items[blockIdx.x];
    bool diff = out_len[blockIdx.x] != it.ref_len;
    if (!diff)
        for (uint32_t i = threadIdx.x; i < it.ref_len; i += blockDim.x) diff |= out[it.out_off + i] != ref[it.ref_off + i];
    if (diff) atomicOr(flags + it.image, 2u);
}

// The launches of the three check kernels, once: launch_compress_chunk and the test hooks (lep_batch_debug_compare, lep_batch_debug_scan_check)
// both go through these, so a test runs the product's grid, block and arguments and not a copy of them.
void launch_compare(const void* a, const void* b, size_t bytes, uint32_t* flag, uint32_t value, hipStream_t st) {
    hipLaunchKernelGGL(lep_compare_kernel, dim3(256), dim3(256), 0, st, (const uint4*)a, (const uint4*)b, bytes / 16, flag, value);
}
// one workgroup of 256 per item (n > 0)
void launch_scan_check_bytes(const uint8_t* out, const uint32_t* out_len, const uint8_t* ref, const ScanCheck* items, unsigned n, uint32_t* flags, hipStream_t st) {
    hipLaunchKernelGGL(lep_scan_check_bytes_kernel, dim3(n), dim3(256), 0, st, out, out_len, ref, items, flags);
}
void launch_scan_check(const uint8_t* out, const uint32_t* out_len, const uint8_t* ref, const ScanCheck* items, unsigned n, uint32_t* flags, hipStream_t st) {
    hipLaunchKernelGGL(lep_scan_check_kernel, dim3(n), dim3(256), 0, st, out, out_len, ref, items, flags);
}

// test hook (lep_batch_debug_tamper): one lane XORs one byte
__global__ void lep_debug_xor_kernel(uint8_t* p, uint32_t mask) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *p = (uint8_t)(*p ^ mask);
}

// Hundreds of host threads each allocating and freeing MB-sized vectors (un-stuffed scan data, containers) serialise on
// the process-wide mmap lock when glibc serves them with mmap/munmap; keep such blocks inside the per-thread arenas.
void tune_malloc_for_pool() {
    static std::atomic<bool> done(false);
    if (done.exchange(true)) return;
    mallopt(M_MMAP_THRESHOLD, 256 << 20);
    mallopt(M_TRIM_THRESHOLD, 512 << 20);
    mallopt(M_ARENA_MAX, 512);
}

// Every buffer of a slot, once -- X(Dev | Pin, type, name, counted): Slot declares them from this list, and release / footprint /
// poison walk it.  `counted`: pinned memory, or one of the large device arenas (lep_batch_footprint; the per-segment tables are KBs)
#define LEP_SLOT_BUFFERS(X)                                                                                                                  \
    X(Dev, char, d_frames, 1)     X(Pin, char, h_frames, 1)                                                                                  \
    X(Dev, char, d_scratch, 1)         /* the verification decode's frames: as large as d_frames, only allocated when asked for */           \
    X(Dev, uint8_t, d_streams, 1) X(Pin, uint8_t, h_streams, 1)   /* device arena (worst-case sized for encode) / pinned mirror (actual bytes) */ \
    X(Dev, uint32_t, d_len, 0)    X(Dev, int32_t, d_status, 0)   /* d_status: [nseg] coder statuses + [nseg] verification-decode statuses */ \
    X(Dev, uint32_t, d_flags, 0)                                                                                                             \
    X(Dev, uint8_t, d_scan, 1)    X(Pin, uint8_t, h_scan, 1)   /* JPEG scan bytes of the GPU Huffman encoder */                              \
    X(Dev, uint32_t, d_scanlen, 0)     /* nseg byte counts, then (16-byte aligned) nseg lep_huff_end records */                              \
    X(Dev, lep_huffdec_row, d_rows, 1) /* row records of the GPU Huffman decoder */                                                          \
    X(Dev, uint8_t, d_pscan, 1)        /* progressive files: the scans' device arena (sized for the worst case) ... */                       \
    X(Pin, uint8_t, h_pscan, 1)        /* ... and the pinned mirror, packed by the bytes actually written */                                 \
    X(Dev, uint32_t, d_corr, 1)        /* held-back correction bits of the refinement scans (dwords) */                                      \
    X(Dev, uint32_t, d_pscanlen, 0)    X(Dev, ScanCheck, d_pcheck, 0)   /* compression with verify: what lep_scan_check_kernel compares */   \
    X(Dev, uint8_t, d_vscan, 1)        /* ... and for baseline files: their scans written again from the device frame, */                    \
    X(Dev, uint32_t, d_vscanlen, 0)    X(Dev, ScanCheck, d_vcheck, 0)   /* per thread segment */

struct Slot {   // one chunk's buffers (double-buffered)
#define X(kind, T, name, counted) lepbuf::kind##Buf<T> name;
    LEP_SLOT_BUFFERS(X)
#undef X
    hipEvent_t up = nullptr, done = nullptr, decoded = nullptr;
    bool done_recorded = false;   // `done` has been recorded in the current batch call
    void release() {
#define X(kind, T, name, counted) (void)name.release();
        LEP_SLOT_BUFFERS(X)
#undef X
        if (up) (void)hipEventDestroy(up);
        if (done) (void)hipEventDestroy(done);
        if (decoded) (void)hipEventDestroy(decoded);
        *this = Slot();
    }
};

#define HIPOK(call) do { if ((call) != hipSuccess) return LEP_GPU_ERROR; } while (0)
// device memory for the pipeline's staging: when the device has none left, what the codec object caches between launches
// (models, the split-phase encoder's scratch -- re-acquired on demand) is given back first
static lep_gpu* g_batch_gpu = nullptr;   // the codec object of the batch call in progress
static hipError_t dev_alloc(void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory && g_batch_gpu) {
        (void)hipGetLastError();
        (void)lep_gpu_release_memory(g_batch_gpu);
        e = hipMalloc(p, bytes);
    }
    if (e != hipSuccess) *p = nullptr;
    return e;
}

struct Joiner {   // a background thread that is joined on every way out of the function, error returns included
    std::thread t;
    ~Joiner() { if (t.joinable()) t.join(); }
};

struct StreamSet {   // HIP streams of one batch call, destroyed on every way out
    std::vector<hipStream_t> all;
    lep_gpu* g = nullptr;   // the codec whose launch functions were handed these streams: its upload ring forgets them first
    int make(hipStream_t* s, int priority = 0, bool with_priority = false) {
        const hipError_t e = with_priority ? hipStreamCreateWithPriority(s, hipStreamNonBlocking, priority) : hipStreamCreateWithFlags(s, hipStreamNonBlocking);
        if (e != hipSuccess) return LEP_GPU_ERROR;
        all.push_back(*s);
        return 0;
    }
    ~StreamSet() {
        for (hipStream_t s : all) (void)hipStreamSynchronize(s);
        if (g) (void)lep_gpu_settle_uploads(g);
        for (hipStream_t s : all) (void)hipStreamDestroy(s);
    }
};
template <class T, void (*CLOSE)(T*)>
struct HandleVector {   // parsed files of a batch: whatever is still open when the call returns is closed
    std::vector<T*> v;
    explicit HandleVector(size_t n) : v(n, nullptr) {}
    ~HandleVector() { for (T* p : v) if (p) CLOSE(p); }
    T*& operator[](size_t i) { return v[i]; }
};

double g_alloc_s = 0;   // time spent in (re)allocating staging buffers during the current call (single orchestrator thread)
struct AllocTimer {
    const double t0 = now_s();
    ~AllocTimer() { g_alloc_s += now_s() - t0; }
};
// a slot's device buffers ask for exactly what they need
template <class T> hipError_t grow(lepbuf::DevBuf<T>& b, size_t need) { return b.ensure(need, 0, dev_alloc); }

// host_streams: bytes of the pinned mirror of the stream arena (decompress: all of it; compress: reserved later, once the
// encoder has reported how many bytes it really wrote -- the arena itself is sized for the worst case, 5x more)
int slot_reserve(Slot* s, size_t frames, size_t streams, size_t nseg, size_t nimg, bool scratch, size_t host_streams) {
    AllocTimer timed;
    if (frames > s->d_frames.cap) (void)s->d_scratch.release();   // (as large as d_frames: it goes when that grows)
    HIPOK(grow(s->d_frames, frames));
    if (scratch) HIPOK(grow(s->d_scratch, s->d_frames.cap));
    HIPOK(grow(s->d_streams, streams));
    HIPOK(s->h_streams.ensure(host_streams, host_streams / 4));   // head room: the next chunk of similar files should not reallocate
    HIPOK(grow(s->d_len, nseg * 4));
    HIPOK(grow(s->d_status, nseg * 8));
    HIPOK(grow(s->d_flags, nimg * 4));
    if (!s->up) HIPOK(hipEventCreateWithFlags(&s->up, hipEventDisableTiming));
    if (!s->done) HIPOK(hipEventCreateWithFlags(&s->done, hipEventDisableTiming));
    if (!s->decoded) HIPOK(hipEventCreateWithFlags(&s->decoded, hipEventDisableTiming));
    return 0;
}

// the end-state records of a launch of nseg segments live behind its byte counts in the same allocation (16-byte aligned)
lep_huff_end* huff_ends(Slot* s, size_t nseg) { return s->d_scanlen.at<lep_huff_end>(lepbuf::round_up(nseg * 4, 16)); }

int scan_reserve(Slot* s, size_t bytes, size_t nseg) {
    AllocTimer timed;
    HIPOK(s->h_scan.ensure(bytes));
    HIPOK(grow(s->d_scan, bytes));
    HIPOK(grow(s->d_scanlen, nseg ? nseg * 4 + 16 + nseg * sizeof(lep_huff_end) : 0));
    return 0;
}
int prog_reserve(Slot* s, size_t scan_bytes, size_t corr_words, size_t nscan) {
    AllocTimer timed;
    HIPOK(grow(s->d_pscan, scan_bytes));
    HIPOK(grow(s->d_corr, corr_words * 4));
    HIPOK(grow(s->d_pscanlen, nscan * 4));
    HIPOK(grow(s->d_pcheck, nscan * sizeof(ScanCheck)));
    return 0;
}
int vscan_reserve(Slot* s, size_t bytes, size_t nseg) {
    AllocTimer timed;
    HIPOK(grow(s->d_vscan, bytes));
    HIPOK(grow(s->d_vscanlen, nseg * 4));
    HIPOK(grow(s->d_vcheck, nseg * sizeof(ScanCheck)));
    return 0;
}
// pinned staging that is only taken where a path needs it: whole frames for the files the host Huffman coder handles (head 0), the
// progressive scans' mirror (a quarter of head room, like h_streams)
template <class T> int pinned_reserve(lepbuf::PinBuf<T>& b, size_t need, size_t head = 0) {
    AllocTimer timed;
    HIPOK(b.ensure(need, head));
    return 0;
}

struct Chunk {
    int first = 0, count = 0;
    std::vector<int> live;                 // indices (into the batch) of the images that go to the GPU
    std::vector<lep_image_desc> host_desc, dev_desc, scratch_desc;
    std::vector<size_t> frame_off;         // per live image: offset of its frame in the slot
    std::vector<lep_segment> segs;
    std::vector<uint64_t> offs;            // stream arena offsets (nseg + 1)
    std::vector<int> seg_first;            // per live image: first segment index
    size_t frame_bytes = 0;
    // decompression: GPU Huffman re-encode plan
    std::vector<lep_huff_image> himg;      // eligible images only
    std::vector<lep_huff_segment> hseg;
    std::vector<int> hfirst;               // per live image: first entry of hseg, -1 = host re-coder
    std::vector<uint32_t> hslot;           // per hseg: bytes reserved in the scan arena
    std::vector<uint32_t> hbound;          // per hseg: the segment's real byte bound (larger than the slot for segment 0)
    size_t scan_bytes = 0;
    // decompression of progressive files: one GPU wavefront per (image, scan) (lep_huffprog.h)
    std::vector<lep_huffprog_image> pimg;
    std::vector<lep_huffprog_scan> pscan;
    std::vector<int> pfirst, pcount;       // per live image: first entry of pscan / number of scans, -1 = not on this path
    size_t pscan_bytes = 0, corr_words = 0;
    std::vector<ScanCheck> pcheck;         // compression with verify: per pscan entry, the file's own bytes of that scan
    // compression with verify, baseline files the GPU decoded: the Huffman half of the round trip (their scans written again)
    std::vector<lep_huff_image> vimg;
    std::vector<lep_huff_segment> vseg;
    std::vector<ScanCheck> vcheck;
    std::vector<char> vchecked;            // per live image: its scan goes through that check
    size_t vscan_bytes = 0;
    std::vector<char> pchecked;            // per live image: its scans go through the progressive check (one flag per image: the writer
                                           // used to scan `pcheck` for every image, images x scans comparisons per chunk -- ADVICE round 3)
};

Slot g_slots[2];         // one batch call at a time (the calls are not re-entrant)

// exact bytes of a coefficient frame (a multiple of 128); a frame's ROOM in a slot is this rounded up to 256
size_t frame_exact_bytes(const lep_image_desc& d) {
    size_t b = 0;
    for (int c = 0; c < d.ncomp; ++c) b += lepbatch::desc_blocks(d, c) * 128;
    return b;
}
size_t frame_bytes_of(const lep_image_desc& d) { return lepbuf::round_up(frame_exact_bytes(d)); }

// a frame descriptor's component pointers into the frame at `frame`, by the geometry of `geo`
template <class Ptr, size_t N> void point_into_frame(Ptr (&blocks)[N], const lep_image_desc& geo, char* frame) {
    lepbatch::point_components(blocks, geo.ncomp, frame, [&](int c) { return lepbatch::desc_blocks(geo, c); });
}

// What the stages of one batch call share.  (Orchestrator thread and writer thread: the writer adds to st.write_s, sets status[] / outs[] of
// the files it writes and closes their handles; everything else is the orchestrator's.)
struct BatchCall {
    lep_gpu* g = nullptr;
    int n = 0;
    lep_bytes* outs = nullptr;
    int32_t* status = nullptr;
    int threads = 1;
    bool gpu_huffman = true;
    bool cut_progressive = false;      // lep_gpu_cut_progressive: progressive files that end inside a scan take the scan kernels
    const bool trace = getenv("LEP_BATCH_TRACE") != nullptr;   // read once per call
    lep_batch_stats st;
    double t_pipe0 = 0;
    StreamSet streams;   // (in front of the file handles: they are closed first, then the streams drained and destroyed)
    BatchCall() { memset(&st, 0, sizeof st); }
};

// ---- JPEG -> .lep, batch ---------------------------------------------------------------------------------------------
struct CompressCall : BatchCall {
    const lep_bytes* jpgs = nullptr;   // bounded by -trunc
    const size_t* start = nullptr;     // -startbyte per file
    bool verify = false, overlap = false;
    hipStream_t s_copy = nullptr, s_compute[2] = {nullptr, nullptr}, s_down = nullptr, s_huff = nullptr;
    HandleVector<lep_jpeg, lep_jpeg_close> parsed;
    std::vector<char> host_parsed;     // files the host parser took (irregular scans): verify also re-codes them on the host
    explicit CompressCall(int n_) : parsed((size_t)n_), host_parsed((size_t)n_, 0) { n = n_; }
};

// One live image of a chunk while it is parsed: route, descriptors, check plan, and (base) its places in the scan arena.
struct LiveImage : lepbatch::ScanArenaImage {
    int file = 0;                                  // index into the batch
    size_t frame_off = 0, frame_room = 0;          // its frame in the slot
    lep_image_desc desc = {};                      // geometry (the frame of a GPU-routed image only exists on the device)
    bool need_host = false;                        // route kHost: the host parser takes it (false: refused outright, it has no route)
    bool redo = false;                             // the GPU decoders refused it: parsed again on the host
    lep_huffdec_image himg = {};                   // sequential: as parsed, then as launched
    uint32_t ref_first = 0;                        // ... and where its scan stands in the file (verify)
    std::vector<lep_huffprogdec_scan> pscans;      // progressive: as parsed, then as launched
    struct { lep_huffprog_image img; std::vector<lep_huffprog_scan> scans; std::vector<uint32_t> first, len; } pchk = {};   // ... and the check's plan (verify)
    bool on_gpu() const { return route != lepbatch::kHost; }
};

// host Huffman decode of a live image into its pinned frame
int host_parse_one(CompressCall& x, Slot* s, LiveImage& im) {
    const int i = im.file;
    lep_jpeg*& pj = x.parsed[i];
    if (pj) { lep_jpeg_close(pj); pj = nullptr; }
    int rc = lep_jpeg_open_slice_into(x.jpgs[i].data, x.jpgs[i].len, x.start[i], s->h_frames + im.frame_off, im.frame_room, &pj);   // (start 0: lep_jpeg_open_into)
    x.host_parsed[i] = 1;
    if (!rc) {
        lep_jpeg_describe(pj, &im.desc);
        const lep_image_desc& d = im.desc;
        if ((char*)d.blocks[0] != s->h_frames + im.frame_off) {   // SOF peek disagreed with the parser: copy into place
            if (frame_bytes_of(d) > im.frame_room) rc = LEP_ASSERTION_FAILURE;
            else {
                size_t off = im.frame_off;
                for (int cc = 0; cc < d.ncomp; ++cc) {
                    const size_t b = lepbatch::desc_blocks(d, cc) * 128;
                    memcpy(s->h_frames + off, d.blocks[cc], b);
                    off += b;
                }
            }
        }
    }
    if (rc) { x.status[i] = rc; if (pj) { lep_jpeg_close(pj); pj = nullptr; } }
    return rc;
}

// stage 1: which decoder takes each file -- the sequential or the progressive one on the GPU, or the host parser (which then runs here)
// Progressive files: their scans go to the GPU scan decoder too (lep_huffprogdec.h).  When the caller wants the round trip verified, the
// Huffman half of that check is made on the GPU as well: every scan of the frame is written again (lep_huffprog.h, the decompressor's
// kernel) and compared with the file's own bytes (no "canonical by construction" argument is made for these scans, unlike the
// sequential kernel's), so a progressive file is only routed to the GPU under `verify` if that check can be planned for it.
int route_chunk(CompressCall& x, Chunk* c, Slot* s, std::vector<LiveImage>& imgs) {
    const int nl = (int)c->live.size();
    imgs.clear(); imgs.resize((size_t)nl);
    for (int k = 0; k < nl; ++k) {
        imgs[k].file = c->live[k]; imgs[k].frame_off = c->frame_off[k]; imgs[k].need_host = !x.gpu_huffman;
        imgs[k].frame_room = (k + 1 < nl ? c->frame_off[k + 1] : c->frame_bytes) - c->frame_off[k];
    }
    if (x.gpu_huffman)
        parallel_for(nl, x.threads, [&](int k) {
            LiveImage& im = imgs[k];
            const int i = im.file;
            int ok = 0;
            int rc = lep_jpeg_open_gpu_slice(x.jpgs[i].data, x.jpgs[i].len, x.start[i], &x.parsed[i], &im.himg, &ok);
            if (rc) { x.status[i] = rc; return; }      // not a JPEG the reference would take either: no route at all
            if (ok) { im.route = lepbatch::kSequential; return; }
            im.pscans.resize(64);
            int ns = 0, okp = 0;
            if (!(x.cut_progressive ? lep_jpeg_open_gpu_progressive_cut : lep_jpeg_open_gpu_progressive)(x.parsed[i], im.pscans.data(), 64, &ns, &im.prow_need, &okp) && okp) {
                im.pscans.resize((size_t)ns);
                if (!x.verify) { im.route = lepbatch::kProgressive; return; }
                auto& pc = im.pchk;
                pc.scans.resize((size_t)ns); pc.first.resize((size_t)ns); pc.len.resize((size_t)ns);
                int nc = 0, okc = 0;
                if (!(x.cut_progressive ? lep_jpeg_plan_progressive_check_cut : lep_jpeg_plan_progressive_check)(x.parsed[i], x.jpgs[i].len, &pc.img, pc.scans.data(), pc.first.data(), pc.len.data(), ns, &nc, &okc) &&
                    okc && nc == ns) { im.route = lepbatch::kProgressive; return; }
            }
            im.pscans.clear();
            im.need_host = true;
        });
    bool any_host = false;
    for (const LiveImage& im : imgs) any_host |= im.need_host;
    if (any_host) {
        if (int rc = pinned_reserve(s->h_frames, c->frame_bytes)) return rc;
        parallel_for(nl, x.threads, [&](int k) { if (imgs[k].need_host) host_parse_one(x, s, imgs[k]); });
    }
    return 0;
}

// stage 2: the scan arena (pinned -> device) and the row records: every GPU-routed scan gets its place (lepbatch::lay_out_scan_arena),
// then the host pool copies scan bytes, restart positions and -- for the round-trip check -- the file's own bytes to where the layout says
int fill_scan_arena(CompressCall& x, Slot* s, std::vector<LiveImage>& imgs, lepbatch::ScanArenaTotals* totals, int* ngpu) {
    for (LiveImage& im : imgs) {
        lep_jpeg* pj = x.parsed[im.file];
        if (im.route == lepbatch::kSequential) {
            im.scan_len = im.himg.scan_len; im.mcuv = im.himg.mcuv;
            im.restarts = (im.himg.flags & LEP_HUFFDEC_RST_TABLE) ? (size_t)((im.himg.mcuc - 1) / im.himg.rsti) : 0;
            uint32_t len = 0;   // baseline files: the whole scan as it stands in the file, for the round-trip check
            if (x.verify && !lep_jpeg_scan_file_range(pj, &im.ref_first, &len)) im.ref_len = len;
        } else if (im.route == lepbatch::kProgressive) {
            im.scans.resize(im.pscans.size());
            for (size_t q = 0; q < im.pscans.size(); ++q) {
                im.scans[q].scan_len = im.pscans[q].t.scan_len;
                if (im.pscans[q].t.flags & LEP_HUFFDEC_RST_TABLE) {   // the restart positions behind the scan's slot (lep_huffprogdec_rst.h)
                    const uint32_t* rp = nullptr;
                    lep_jpeg_scan_restarts_of(pj, (int)q, &rp, &im.scans[q].restarts);
                }
                if (x.verify) im.scans[q].ref_len = im.pchk.len[q];
            }
        }
        *ngpu += im.on_gpu();
    }
    *totals = lepbatch::lay_out_scan_arena(imgs.data(), imgs.size(), x.verify);
    if (!*ngpu) return 0;
    if (int rc = scan_reserve(s, totals->scan_total + 256, 0)) return rc;
    { AllocTimer timed; HIPOK(grow(s->d_rows, totals->rows_total * sizeof(lep_huffdec_row))); }
    parallel_for((int)imgs.size(), x.threads, [&](int k) {
        const LiveImage& im = imgs[k];
        if (!im.on_gpu()) return;
        lep_jpeg* pj = x.parsed[im.file];
        const uint8_t *p = nullptr, *file = x.jpgs[im.file].data;
        size_t len = 0;
        lep_jpeg_scan_bytes(pj, &p, &len);
        const uint32_t* rp = nullptr; size_t rn = 0;
        if (im.route == lepbatch::kProgressive) {
            for (size_t q = 0; q < im.scans.size(); ++q) {
                const lepbatch::ScanPlace& at = im.scans[q];
                const size_t off = (size_t)(uintptr_t)im.pscans[q].t.scan, n = at.scan_len;
                memcpy(s->h_scan + at.off, p + off, n);
                memset(s->h_scan + at.off + n, 0, at.table_off - at.off - n);
                if (im.pscans[q].t.flags & LEP_HUFFDEC_RST_TABLE) {
                    lep_jpeg_scan_restarts_of(pj, (int)q, &rp, &rn);
                    memcpy(s->h_scan + at.table_off, rp, rn * 4);
                }
                if (x.verify) memcpy(s->h_scan + at.ref_off, file + im.pchk.first[q], at.ref_len);
            }
            return;
        }
        memcpy(s->h_scan + im.scan_off, p, len);
        memset(s->h_scan + im.scan_off + len, 0, im.table_off - im.scan_off - len);
        if (im.himg.flags & LEP_HUFFDEC_RST_TABLE) {
            lep_jpeg_scan_restarts(pj, &rp, &rn);
            memcpy(s->h_scan + im.table_off, rp, rn * 4);
        }
        if (im.ref_len) memcpy(s->h_scan + im.ref_off, file + im.ref_first, im.ref_len);
    });
    return 0;
}

// stage 3: uploads -- zero frames for the GPU-decoded images, host-decoded frames as they are, the scan arena
int upload_chunk(CompressCall& x, Chunk* c, Slot* s, const std::vector<LiveImage>& imgs, size_t scan_total, int ngpu) {
    HIPOK(hipMemsetAsync(s->d_frames, 0, c->frame_bytes, x.s_copy));
    // (exactly the frame: the parser zeroes and fills frame_exact_bytes only, the rest of the 256-byte-rounded room in the
    // pinned staging is whatever an earlier batch left there and must not reach the device, where the padding stays zero)
    for (const LiveImage& im : imgs) if (!im.on_gpu() && x.parsed[im.file]) {
        const size_t fb = frame_exact_bytes(im.desc);
        HIPOK(hipMemcpyAsync(s->d_frames + im.frame_off, s->h_frames + im.frame_off, fb, hipMemcpyHostToDevice, x.s_copy));
        x.st.h2d_bytes += (double)fb;
    }
    if (!ngpu) return 0;
    HIPOK(hipMemcpyAsync(s->d_scan, s->h_scan, scan_total, hipMemcpyHostToDevice, x.s_copy));
    x.st.h2d_bytes += (double)scan_total;
    HIPOK(hipEventRecord(s->up, x.s_copy));
    return 0;
}

// the one "copy the row records down and wait"
int fetch_rows(CompressCall& x, Slot* s, std::vector<lep_huffdec_row>& rows) {
    HIPOK(hipMemcpyAsync(rows.data(), s->d_rows, rows.size() * sizeof(lep_huffdec_row), hipMemcpyDeviceToHost, x.s_huff));
    HIPOK(hipStreamSynchronize(x.s_huff));
    return 0;
}

// stage 4a: Huffman scan decode of the sequential files on the GPU: one LANE per subsequence (lep_huffdec_simt.h: thousands of
// subsequences per scan, 64 codes per instruction) for the scans without restart intervals, the single-wave kernel (lep_huffdec.h)
// for the others; lanes = false (LEP_HUFFDEC_SIMT=0) keeps the single-wave kernel for every file.  (Round 2-4's form in between --
// several WAVEFRONTS per image, 290 ms per 896-file chunk against 43 -- is gone from the product: LAB_NOTES.md 4 "JPEG Huffman
// kernels" keeps its numbers.)  `launch`: the descriptors as they went out.
int run_sequential_decoders(CompressCall& x, Slot* s, std::vector<LiveImage>& imgs, bool lanes, std::vector<lep_huffdec_image>& launch) {
    for (LiveImage& im : imgs) if (im.route == lepbatch::kSequential) {
        lep_huffdec_image& hi = im.himg;
        hi.scan = s->d_scan + im.scan_off;
        hi.rows_off = im.row_off;
        lepbatch::point_components(hi.blocks, hi.ncomp, s->d_frames + im.frame_off, [&](int cc) { return (size_t)hi.bch[cc] * hi.vs[cc] * hi.mcuv; });
        launch.push_back(hi);
    }
    HIPOK(hipStreamWaitEvent(x.s_huff, s->up, 0));
    if (!lanes) return lep_gpu_huffman_decode_device(x.g, launch.data(), (int)launch.size(), s->d_rows, x.s_huff);
    std::vector<lep_huffdec_image> many, one;
    for (const lep_huffdec_image& hi : launch) (lephuff::simt_dec_takes(hi) ? many : one).push_back(hi);
    if (!many.empty()) { if (int rc = lep_gpu_huffman_decode_simt_device(x.g, many.data(), (int)many.size(), s->d_rows, x.s_huff)) return rc; }
    if (!one.empty()) { if (int rc = lep_gpu_huffman_decode_device(x.g, one.data(), (int)one.size(), s->d_rows, x.s_huff)) return rc; }
    return 0;
}
// a scan whose subsequences did not synchronise (or that is irregular) gets a second chance with the single-wave kernel before the
// host parser is bothered: its frame is wiped first (pass C may have written part of it)
int second_chance_sequential(CompressCall& x, Slot* s, const std::vector<lep_huffdec_image>& launch, std::vector<lep_huffdec_row>& rows) {
    std::vector<lep_huffdec_image> again;
    for (const lep_huffdec_image& hi : launch) {
        if (!lephuff::simt_dec_takes(hi) || ((rows[hi.rows_off + (size_t)hi.mcuv].aux >> 8) & 0x3fffff) == 0) continue;   // (bit 30: LEP_HUFFDEC_ROW_TRUNCATED, not a status)
        for (int cc = 0; cc < hi.ncomp; ++cc)
            HIPOK(hipMemsetAsync(hi.blocks[cc], 0, (size_t)hi.bch[cc] * hi.vs[cc] * hi.mcuv * 128, x.s_huff));
        again.push_back(hi);
    }
    if (again.empty()) return 0;
    g_scan_second_chances.fetch_add((uint64_t)again.size(), std::memory_order_relaxed);
    if (int rc = lep_gpu_huffman_decode_device(x.g, again.data(), (int)again.size(), s->d_rows, x.s_huff)) return rc;
    return fetch_rows(x, s, rows);
}

// stage 4b: progressive files: one wavefront per (image, scan), launched dependency level by dependency level
int run_progressive_decoders(CompressCall& x, Slot* s, std::vector<LiveImage>& imgs) {
    std::vector<lep_huffprogdec_scan> plaunch;
    for (LiveImage& im : imgs) if (im.route == lepbatch::kProgressive)
        for (size_t q = 0; q < im.pscans.size(); ++q) {
            lep_huffprogdec_scan& sc = im.pscans[q];
            sc.t.scan = s->d_scan + im.scans[q].off;
            lepbatch::point_components(sc.t.blocks, sc.t.ncomp, s->d_frames + im.frame_off, [&](int cc) { return (size_t)sc.t.bch[cc] * sc.bcv[cc]; });
            sc.t.rows_off += im.row_off;
            sc.result_off += im.row_off;
            plaunch.push_back(sc);
        }
    if (plaunch.empty()) return 0;
    return lep_gpu_huffman_progressive_decode_device(x.g, plaunch.data(), (int)plaunch.size(), s->d_rows, x.s_huff);
}
// A progressive file in which a scan decoded interval by interval (lep_huffprogdec_rst.h) ended with a status gets a second chance
// with the older forms before the host parser is bothered, its frame wiped first: an interval of a damaged file that does not end
// at its marker is something the reference, which never looks at where the markers stood, may still decode.
int second_chance_progressive(CompressCall& x, Slot* s, std::vector<LiveImage>& imgs, std::vector<lep_huffdec_row>& rows) {
    std::vector<lep_huffprogdec_scan> again;
    for (LiveImage& im : imgs) if (im.route == lepbatch::kProgressive) {
        bool bad = false;
        for (const lep_huffprogdec_scan& sc : im.pscans) bad = bad || ((sc.t.flags & LEP_HUFFDEC_RST_TABLE) && (rows[sc.result_off].aux >> 8) != 0);
        if (!bad) continue;
        size_t fb = 0;
        const lep_huffprogdec_scan& f = im.pscans[0];
        for (int cc = 0; cc < f.t.ncomp; ++cc) fb += (size_t)f.t.bch[cc] * f.bcv[cc] * 128;
        HIPOK(hipMemsetAsync(s->d_frames + im.frame_off, 0, fb, x.s_huff));
        for (lep_huffprogdec_scan& sc : im.pscans) {
            sc.t.flags &= ~LEP_HUFFDEC_RST_TABLE;      // (the contract of the flag: cleared, the scan goes to lep_huffprogdec.h)
            again.push_back(sc);
        }
    }
    if (again.empty()) return 0;
    if (int rc = lep_gpu_huffman_progressive_decode_device(x.g, again.data(), (int)again.size(), s->d_rows, x.s_huff)) return rc;
    return fetch_rows(x, s, rows);
}

// stage 5: hand-offs from the row records; irregular scans go back to the host parser (and their frames up again)
int finish_handoffs(CompressCall& x, Chunk* c, Slot* s, std::vector<LiveImage>& imgs, const std::vector<lep_huffdec_row>& rows) {
    const double t0 = now_s();
    parallel_for((int)imgs.size(), x.threads, [&](int k) {
        LiveImage& im = imgs[k];
        lep_jpeg* pj = x.parsed[im.file];
        if (!im.on_gpu()) return;
        if (im.route == lepbatch::kProgressive ? lep_jpeg_finish_gpu_progressive(pj, im.pscans.data(), (int)im.pscans.size(), rows.data())
                                               : lep_jpeg_finish_gpu(pj, rows.data() + im.row_off)) { im.redo = true; im.route = lepbatch::kHost; return; }
        lep_jpeg_describe(pj, &im.desc);   // geometry; the frame itself only exists on the device
    });
    bool any_redo = false;
    for (const LiveImage& im : imgs) any_redo |= im.redo;
    if (any_redo) {
        if (int rc = pinned_reserve(s->h_frames, c->frame_bytes)) return rc;
        parallel_for((int)imgs.size(), x.threads, [&](int k) { if (imgs[k].redo) host_parse_one(x, s, imgs[k]); });
    }
    x.st.parse_s += now_s() - t0;
    for (const LiveImage& im : imgs) if (im.redo && x.parsed[im.file]) {
        const size_t fb = frame_exact_bytes(im.desc);   // the whole frame: the GPU decoder may have written part of it
        HIPOK(hipMemcpyAsync(s->d_frames + im.frame_off, s->h_frames + im.frame_off, fb, hipMemcpyHostToDevice, x.s_copy));
        x.st.h2d_bytes += (double)fb;
    }
    return 0;
}

// stage 6: drop failed images from the chunk (their records go with them), then thread segments and their slots in the stream arena.
// What still overflows its slot is redone per file (redo_overflowed).
int plan_segments(CompressCall& x, Chunk* c, std::vector<LiveImage>& imgs) {
    size_t kept = 0;
    for (size_t k = 0; k < imgs.size(); ++k) if (x.parsed[imgs[k].file]) { if (kept != k) imgs[kept] = std::move(imgs[k]); ++kept; }
    imgs.resize(kept);
    c->live.clear(); c->frame_off.clear(); c->host_desc.clear();
    for (const LiveImage& im : imgs) { c->live.push_back(im.file); c->frame_off.push_back(im.frame_off); c->host_desc.push_back(im.desc); }
    c->segs.clear(); c->offs.assign(1, 0); c->seg_first.clear();
    for (size_t k = 0; k < c->live.size(); ++k) {
        lep_jpeg* pj = x.parsed[c->live[k]];
        lep_segment sg[LEP_MAX_SEGMENTS];
        lep_handoff ho[LEP_MAX_SEGMENTS];
        const int ns = lep_jpeg_plan(pj, 0, sg, (int)k);
        if (lep_jpeg_plan_handoffs(pj, 0, ho, LEP_MAX_SEGMENTS) != ns || ns < 0) return LEP_ASSERTION_FAILURE;   // (the two plans are one choice; ho[] is read below)
        c->seg_first.push_back((int)c->segs.size());
        const lep_image_desc& d = c->host_desc[k];
        size_t blocks = 0;
        for (int cc = 0; cc < d.ncomp; ++cc) blocks += lepbatch::desc_blocks(d, cc);
        const bool prog = lep_jpeg_is_progressive(pj) != 0;
        for (int q = 0; q < ns; ++q) {
            c->segs.push_back(sg[q]);
            c->offs.push_back(c->offs.back() + lepbatch::stream_slot_bytes(ho[q].segment_size, blocks, ns, prog));
        }
    }
    c->seg_first.push_back((int)c->segs.size());
    return 0;
}

// stage 7a: round-trip check of the progressive files the GPU decoded: their scans written again from the device frame
void plan_progressive_check(CompressCall& x, Chunk* c, Slot* s, const std::vector<LiveImage>& imgs) {
    c->pimg.clear(); c->pscan.clear(); c->pcheck.clear();
    c->pchecked.assign(c->live.size(), 0);
    lepbatch::OutputArena arena;
    for (size_t k = 0; x.verify && k < imgs.size(); ++k) {
        const LiveImage& im = imgs[k];
        if (im.route != lepbatch::kProgressive) continue;
        lep_huffprog_image pi = im.pchk.img;
        point_into_frame(pi.blocks, c->host_desc[k], s->d_frames + c->frame_off[k]);
        for (size_t q = 0; q < im.pchk.scans.size(); ++q) {
            lep_huffprog_scan sc = im.pchk.scans[q];
            sc.image = (int32_t)c->pimg.size();
            // (the scan a file ends in keeps the cap of its geometry: its writer's buffers are sized from it, and it is written whole)
            const bool ends_here = q < im.pscans.size() && (im.pscans[q].t.flags & LEP_HUFFDEC_EARLY_EOF);
            if (!ends_here) sc.out_cap = lepbatch::verify_out_cap(sc.out_cap, im.pchk.len[q]);
            sc.out_off = arena.place(sc.out_cap);
            sc.corr_off = (uint32_t)arena.place_corr(sc.corr_cap);
            c->pscan.push_back(sc);
            c->pcheck.push_back(ScanCheck{sc.out_off, (uint64_t)im.scans[q].ref_off, im.pchk.len[q], (uint32_t)k | (ends_here ? kScanCheckPrefix : 0u)});
            c->pchecked[k] = 1;
        }
        c->pimg.push_back(pi);
    }
    c->pscan_bytes = arena.bytes; c->corr_words = arena.corr_words;
}
// stage 7b: ... and of the baseline files it decoded (their frame exists only on the device): every thread segment's scan bytes
// written again by the decompressor's kernel and held against the file's.  A file that cannot take this path -- or whose
// bytes do not come back -- goes through the per-file path, which restores it on the host and compares.
void plan_baseline_check(CompressCall& x, Chunk* c, Slot* s, const std::vector<LiveImage>& imgs) {
    c->vimg.clear(); c->vseg.clear(); c->vcheck.clear();
    c->vchecked.assign(c->live.size(), 0);
    lepbatch::OutputArena arena;
    for (size_t k = 0; x.verify && k < imgs.size(); ++k) {
        const LiveImage& im = imgs[k];
        if (im.route != lepbatch::kSequential || !im.ref_len) continue;
        lep_huff_image vi;
        lep_huff_segment vs[LEP_MAX_SEGMENTS];
        uint32_t ff[LEP_MAX_SEGMENTS], fl[LEP_MAX_SEGMENTS];
        int ns = 0, ok = 0;
        if (lep_jpeg_plan_scan_check(x.parsed[im.file], x.jpgs[im.file].len, &vi, vs, ff, fl, LEP_MAX_SEGMENTS, &ns, &ok) || !ok) continue;
        point_into_frame(vi.blocks, c->host_desc[k], s->d_frames + c->frame_off[k]);
        for (int q = 0; q < ns; ++q) {
            vs[q].image = (int32_t)c->vimg.size();
            vs[q].out_cap = lepbatch::verify_out_cap(vs[q].out_cap, fl[q]);
            vs[q].out_off = arena.place(vs[q].out_cap);
            c->vseg.push_back(vs[q]);
            c->vcheck.push_back(ScanCheck{vs[q].out_off, (uint64_t)im.ref_off + (ff[q] - im.ref_first), fl[q], (uint32_t)k});
        }
        c->vimg.push_back(vi);
        c->vchecked[k] = 1;
    }
    c->vscan_bytes = arena.bytes;
}
int upload_checks(CompressCall& x, Chunk* c, Slot* s) {
    if (!c->vseg.empty()) {
        if (int rc = vscan_reserve(s, c->vscan_bytes + 256, c->vseg.size())) return rc;
        HIPOK(hipMemcpyAsync(s->d_vcheck, c->vcheck.data(), c->vcheck.size() * sizeof(ScanCheck), hipMemcpyHostToDevice, x.s_copy));
    }
    if (!c->pscan.empty()) {
        if (c->corr_words > 0xfffffff0u) return LEP_GPU_ERROR;
        if (int rc = prog_reserve(s, c->pscan_bytes + 256, c->corr_words + 16, c->pscan.size())) return rc;
        HIPOK(hipMemcpyAsync(s->d_pcheck, c->pcheck.data(), c->pcheck.size() * sizeof(ScanCheck), hipMemcpyHostToDevice, x.s_copy));
    }
    return 0;
}

// stage 8: a slice's frame rows in front of its first kept hand-off belong to nobody: no thread segment codes them, the decoder leaves
// them zero, no writer reads them.  The scan decoders fill them all the same (first_mcu_row = 0: which rows lie in front of start_byte
// is only known from the records they leave), so they are wiped here, behind every upload and scan decode of the chunk and in
// front of the coder kernels: the frame comparison of `verify` then holds the rows that count and no others.
// (only `verify` looks at them: its frame comparison.  Without it they are left as decoded, as the per-file path leaves them.)
int wipe_slice_rows(CompressCall& x, Chunk* c) {
    for (size_t k = 0; x.verify && k < c->live.size(); ++k) {
        const int i = c->live[k];
        if (!x.start[i]) continue;
        const lep_image_desc& d = c->host_desc[k];
        const int y0 = lep_jpeg_first_kept_luma_row(x.parsed[i]);
        for (int cc = 0; cc < d.ncomp && y0 > 0 && d.height_blocks[0] > 0; ++cc) {
            const size_t rows = std::min<size_t>((size_t)y0 * (size_t)d.height_blocks[cc] / (size_t)d.height_blocks[0], (size_t)d.height_blocks[cc]);
            if (rows) HIPOK(hipMemsetAsync(c->dev_desc[k].blocks[cc], 0, rows * (size_t)d.width_blocks[cc] * 128, x.s_copy));
        }
    }
    return 0;
}

// Per chunk: split the files on the host pool; eligible scans are Huffman-decoded ON THE GPU straight into the device frame (only the
// 2 MB of scan bytes cross PCIe), the others by the host parser into the slot's pinned frames; then the hand-offs are finished,
// segments planned and the upload event recorded
int parse_and_upload(CompressCall& x, Chunk* c, Slot* s) {
    if (c->live.empty()) return 0;
    if (int rc = slot_reserve(s, c->frame_bytes, 0, 0, c->live.size(), x.verify, 0)) return rc;
    const double t0 = now_s();
    std::vector<LiveImage> imgs;
    lepbatch::ScanArenaTotals at;
    int ngpu = 0;
    if (int rc = route_chunk(x, c, s, imgs)) return rc;
    if (int rc = fill_scan_arena(x, s, imgs, &at, &ngpu)) return rc;
    x.st.parse_s += now_s() - t0;
    if (int rc = upload_chunk(x, c, s, imgs, at.scan_total, ngpu)) return rc;
    if (ngpu) {
        std::vector<lep_huffdec_row> rows(at.rows_total);
        const bool lanes = !(getenv("LEP_HUFFDEC_SIMT") && atoi(getenv("LEP_HUFFDEC_SIMT")) == 0);
        std::vector<lep_huffdec_image> seq;
        if (int rc = run_sequential_decoders(x, s, imgs, lanes, seq)) return rc;
        if (int rc = run_progressive_decoders(x, s, imgs)) return rc;
        if (int rc = fetch_rows(x, s, rows)) return rc;
        x.st.d2h_bytes += (double)(rows.size() * sizeof(lep_huffdec_row));
        if (lanes) { if (int rc = second_chance_sequential(x, s, seq, rows)) return rc; }
        if (int rc = second_chance_progressive(x, s, imgs, rows)) return rc;
        if (int rc = finish_handoffs(x, c, s, imgs, rows)) return rc;
    }
    for (const LiveImage& im : imgs) if (im.on_gpu() && x.parsed[im.file]) x.st.gpu_huffman_files += 1;
    if (int rc = plan_segments(x, c, imgs)) return rc;
    if (c->live.empty()) return 0;
    if (int rc = slot_reserve(s, c->frame_bytes, c->offs.back() + 256, c->segs.size(), c->live.size(), x.verify, 0)) return rc;
    c->dev_desc = c->host_desc; c->scratch_desc = c->host_desc;
    for (size_t k = 0; k < c->live.size(); ++k) {
        point_into_frame(c->dev_desc[k].blocks, c->host_desc[k], s->d_frames + c->frame_off[k]);
        if (x.verify) point_into_frame(c->scratch_desc[k].blocks, c->host_desc[k], s->d_scratch + c->frame_off[k]);
    }
    plan_progressive_check(x, c, s, imgs);
    plan_baseline_check(x, c, s, imgs);
    if (int rc = upload_checks(x, c, s)) return rc;
    if (int rc = wipe_slice_rows(x, c)) return rc;
    HIPOK(hipEventRecord(s->up, x.s_copy));
    return 0;
}

// Test hook (lep_batch_debug_tamper): one armed alteration, applied at most once, by the chunk that holds the file, at the stage it names.
struct Tamper {
    bool armed = false;
    int where = 0, file = -1, mask = 0, applied = 0;
    uint64_t offset = 0;
    uint32_t seen_flags = 0;    // what the check then said of that file, as write_containers read it: its flag word ...
    int32_t seen_status = 0;    // ... and the first status of its verification decode that was not zero
};
Tamper g_tamper;
// Where the armed byte lies in the chunk's buffer of stage `where`, or false: another stage, the file is not in this chunk, the call
// has no such buffer, or the offset lies outside what the layout gave that buffer (sizes known on the host before anything is queued).
bool tamper_target(const Tamper& t, bool verify, const Chunk& c, int where, size_t* at) {
    if (!t.armed || t.where != where) return false;
    size_t k = 0;
    while (k < c.live.size() && c.live[k] != t.file) ++k;
    if (k == c.live.size()) return false;
    if (where == LEP_TAMPER_STREAM) {
        const size_t q = (size_t)c.seg_first[k];
        if ((int)q >= c.seg_first[k + 1] || t.offset >= c.offs[q + 1] - c.offs[q]) return false;
        *at = (size_t)(c.offs[q] + t.offset);
        return true;
    }
    if (!verify) return false;
    if (where == LEP_TAMPER_SCRATCH) {
        if (t.offset >= frame_exact_bytes(c.host_desc[k])) return false;
        *at = c.frame_off[k] + (size_t)t.offset;
        return true;
    }
    if (where == LEP_TAMPER_VSCAN) {
        for (size_t q = 0; q < c.vseg.size(); ++q) if (c.vcheck[q].image == (uint32_t)k) {
            if (t.offset >= c.vseg[q].out_cap) return false;
            *at = (size_t)(c.vseg[q].out_off + t.offset);
            return true;
        }
        return false;
    }
    if (where == LEP_TAMPER_PSCAN) {
        for (size_t q = 0; q < c.pscan.size(); ++q) if ((c.pcheck[q].image & ~kScanCheckPrefix) == (uint32_t)k) {
            if (t.offset >= c.pscan[q].out_cap) return false;
            *at = (size_t)(c.pscan[q].out_off + t.offset);
            return true;
        }
        return false;
    }
    return false;
}
hipError_t tamper_chunk(CompressCall& x, Chunk* c, Slot* s, int where, hipStream_t st) {
    size_t at = 0;
    if (!tamper_target(g_tamper, x.verify, *c, where, &at)) return hipSuccess;
    uint8_t* base = (uint8_t*)(where == LEP_TAMPER_STREAM ? s->d_streams.p : where == LEP_TAMPER_SCRATCH ? s->d_scratch.p
                               : where == LEP_TAMPER_VSCAN ? s->d_vscan.p : s->d_pscan.p);
    const size_t cap = where == LEP_TAMPER_STREAM ? s->d_streams.cap : where == LEP_TAMPER_SCRATCH ? s->d_scratch.cap
                     : where == LEP_TAMPER_VSCAN ? s->d_vscan.cap : s->d_pscan.cap;
    if (!base || at >= cap) return hipSuccess;   // (the layout's sizes lie inside the allocations: held once more against the allocation itself)
    g_tamper.armed = false;
    g_tamper.applied += 1;
    hipLaunchKernelGGL(lep_debug_xor_kernel, dim3(1), dim3(64), 0, st, base + at, (uint32_t)(g_tamper.mask & 0xff));
    return hipGetLastError();
}

// coder kernels of one chunk, stream-ordered behind the previous chunk's (the call returns once they are enqueued, i.e.
// after the previous chunk's kernels have finished: the descriptor upload inside lep_gpu_encode_device is synchronous)
int launch_compress_chunk(CompressCall& x, Chunk* c, Slot* s) {
    const int nseg = (int)c->segs.size(), nimg = (int)c->live.size();
    if (!nimg) return 0;
    const int set = x.overlap ? (int)(s - g_slots) : 0;            // slot 0 / 1 <-> stream and workspace set 0 / 1
    hipStream_t s_compute = x.s_compute[set];
    if (int rc0 = lep_gpu_use_arena(x.g, set)) return rc0;
    HIPOK(hipStreamWaitEvent(s_compute, s->up, 0));
    const bool tamper = g_tamper.armed;   // (test hook: the one test an unarmed call pays per chunk)
    int rc = lep_gpu_encode_device(x.g, c->dev_desc.data(), nimg, c->segs.data(), nseg, s->d_streams, c->offs.data(), s->d_len, s->d_status, s_compute);
    if (rc) return rc;
    if (tamper) HIPOK(tamper_chunk(x, c, s, LEP_TAMPER_STREAM, s_compute));
    if (x.verify) {
        HIPOK(hipMemsetAsync(s->d_scratch, 0, c->frame_bytes, s_compute));
        HIPOK(hipMemsetAsync(s->d_flags, 0, (size_t)nimg * 4, s_compute));
        rc = lep_gpu_decode_device(x.g, c->scratch_desc.data(), nimg, c->segs.data(), nseg, s->d_streams, c->offs.data(), s->d_len, s->d_status + nseg, s_compute);
        if (rc) return rc;
        if (tamper) HIPOK(tamper_chunk(x, c, s, LEP_TAMPER_SCRATCH, s_compute));
        for (int k = 0; k < nimg; ++k)   // the frame itself, not its rounded room in the slot
            launch_compare(s->d_frames + c->frame_off[k], s->d_scratch + c->frame_off[k], frame_exact_bytes(c->host_desc[k]), s->d_flags + k, 1u, s_compute);
        x.st.gpu_verified_scans += (double)(c->vseg.size() + c->pscan.size());
        if (!c->vseg.empty()) {    // baseline files: the Huffman half, thread segment by thread segment against the file's bytes
            rc = lep_gpu_huffman_encode_device(x.g, c->vimg.data(), (int)c->vimg.size(), c->vseg.data(), (int)c->vseg.size(), s->d_vscan, s->d_vscanlen, nullptr, s_compute);
            if (rc) return rc;
            if (tamper) HIPOK(tamper_chunk(x, c, s, LEP_TAMPER_VSCAN, s_compute));
            launch_scan_check_bytes(s->d_vscan, s->d_vscanlen, s->d_scan, s->d_vcheck, (unsigned)c->vseg.size(), s->d_flags, s_compute);
        }
        if (!c->pscan.empty()) {   // progressive files: the Huffman half, scan by scan against the file's bytes
            rc = lep_gpu_huffman_progressive_encode_device(x.g, c->pimg.data(), (int)c->pimg.size(), c->pscan.data(), (int)c->pscan.size(), s->d_pscan,
                                                           s->d_corr, s->d_pscanlen, s_compute);
            if (rc) return rc;
            if (tamper) HIPOK(tamper_chunk(x, c, s, LEP_TAMPER_PSCAN, s_compute));
            launch_scan_check(s->d_pscan, s->d_pscanlen, s->d_scan, s->d_pcheck, (unsigned)c->pscan.size(), s->d_flags, s_compute);
        }
    }
    HIPOK(hipEventRecord(s->done, s_compute));
    (void)lep_gpu_use_arena(x.g, 0);
    return 0;
}

struct CompressResults {   // a chunk's results as fetched: copied by value into the writer thread
    std::vector<uint32_t> lens;     // per segment: stream bytes
    std::vector<size_t> hoff;       // per segment: where the stream lies in the pinned mirror
    std::vector<int32_t> sts;       // [nseg] coder statuses + [nseg] verification-decode statuses
    std::vector<uint32_t> flags;    // per image: verification flags
};
int fetch_streams(CompressCall& x, Chunk* c, Slot* s, CompressResults* r) {
    const int nseg = (int)c->segs.size(), nimg = (int)c->live.size();
    r->lens.assign(nseg, 0); r->hoff.assign(nseg, 0); r->sts.assign((size_t)nseg * 2, 0); r->flags.assign(nimg, 0);
    if (!nimg) return 0;
    std::vector<uint32_t>& lens = r->lens;
    std::vector<int32_t>& sts = r->sts;
    HIPOK(hipStreamWaitEvent(x.s_down, s->done, 0));
    HIPOK(hipMemcpyAsync(lens.data(), s->d_len, (size_t)nseg * 4, hipMemcpyDeviceToHost, x.s_down));
    HIPOK(hipMemcpyAsync(sts.data(), s->d_status, (size_t)nseg * (x.verify ? 8 : 4), hipMemcpyDeviceToHost, x.s_down));
    if (x.verify) HIPOK(hipMemcpyAsync(r->flags.data(), s->d_flags, (size_t)nimg * 4, hipMemcpyDeviceToHost, x.s_down));
    HIPOK(hipStreamSynchronize(x.s_down));
    // The streams come down in ONE copy of the arena as it lies on the device (every segment's slot is its JPEG bytes + 25 %, so
    // the slack costs a quarter more PCIe bytes) instead of one copy per segment: 7168 copies of ~200 KB took 250 ms per chunk
    // where their bytes need 30 (kernel + copy trace, profiles/r05b_*) -- and the last chunk's are the call's tail.  An arena
    // that is mostly slack (refused segments, tiny files in generous slots) keeps the packed form.
    size_t total = 0, live_bytes = 0;
    for (int k = 0; k < nseg; ++k) if (!sts[k]) live_bytes += lens[k];
    const size_t extent = nseg ? (size_t)c->offs[nseg] : 0;
    if (lepbatch::download_whole(extent, live_bytes)) {
        for (int k = 0; k < nseg; ++k) r->hoff[k] = (size_t)c->offs[k];
        if (int rc = slot_reserve(s, 0, 0, 0, 0, false, extent + 256)) return rc;
        if (extent) HIPOK(hipMemcpyAsync(s->h_streams, s->d_streams, extent, hipMemcpyDeviceToHost, x.s_down));
        x.st.d2h_bytes += (double)extent;
    } else {
        for (int k = 0; k < nseg; ++k) { r->hoff[k] = total; if (!sts[k]) total += lepbatch::align16(lens[k]); }
        if (int rc = slot_reserve(s, 0, 0, 0, 0, false, total + 256)) return rc;
        for (int k = 0; k < nseg; ++k)
            if (!sts[k] && lens[k]) {
                HIPOK(hipMemcpyAsync(s->h_streams + r->hoff[k], s->d_streams + c->offs[k], lens[k], hipMemcpyDeviceToHost, x.s_down));
                x.st.d2h_bytes += lens[k];
            }
    }
    HIPOK(hipStreamSynchronize(x.s_down));
    return 0;
}

// containers on the host pool (the writer thread)
void write_containers(CompressCall& x, Chunk* c, Slot* s, const CompressResults& r) {
    const double t0 = now_s();
    const std::vector<int32_t>& sts = r.sts;
    parallel_for((int)c->live.size(), x.threads, [&](int k) {
        const int i = c->live[k];
        const int s0 = c->seg_first[k], s1 = c->seg_first[k + 1];
        int rc = 0;
        lep_bytes strs[LEP_MAX_SEGMENTS];
        for (int q = s0; q < s1; ++q) {
            if (sts[q] && !rc) rc = sts[q];
            strs[q - s0].data = s->h_streams + r.hoff[q];
            strs[q - s0].len = strs[q - s0].cap = r.lens[q];
        }
        if (!rc && x.verify) {
            for (int q = s0; q < s1; ++q) if (sts[c->segs.size() + (size_t)q]) rc = LEP_ROUNDTRIP_FAILURE;
            if (g_tamper.applied && g_tamper.file == i) {   // (test hook: which signal the altered file raised)
                g_tamper.seen_flags = r.flags[k];
                for (int q = s1 - 1; q >= s0; --q) if (sts[c->segs.size() + (size_t)q]) g_tamper.seen_status = sts[c->segs.size() + (size_t)q];
            }
            if (r.flags[k] & 1) rc = LEP_ROUNDTRIP_FAILURE;
            // a progressive scan the GPU encoder did not reproduce (trailing restart markers, which the host appends; a
            // non-canonical code choice): the per-file path decides (redo_overflowed)
            else if (!rc && (r.flags[k] & 2)) rc = LEP_BUFFER_TOO_SMALL;
            // a baseline file the GPU decoded whose scan could not go through the check above: the per-file path restores
            // it on the host and compares (nothing is released on an argument)
            else if (!rc && !x.host_parsed[i] && !c->vchecked[k] && !c->pchecked[k]) rc = LEP_BUFFER_TOO_SMALL;
        }
        // a slice at one of the positions the reference's own re-coder does not restore: lep_compress_slice restores every file it
        // writes and names the refusal, so such a slice takes the per-file path whether or not the caller asked for `verify`
        if (!rc && !lep_jpeg_slice_tiles(x.parsed[i])) rc = LEP_BUFFER_TOO_SMALL;
        if (!rc) rc = lep_jpeg_write_lep(x.parsed[i], 0, strs, s1 - s0, &x.outs[i]);
        // the Huffman half of the reference's round-trip check for the files whose scans the host parser took (their
        // frame is still in this slot's pinned staging); the files the GPU decoded had theirs on the GPU (flags, above)
        if (!rc && x.verify && x.host_parsed[i]) {
            rc = lep_jpeg_check_restores(x.parsed[i], x.outs[i].data, x.outs[i].len, x.jpgs[i].data + x.start[i], x.jpgs[i].len - x.start[i]);   // (a slice that parsed: start < len)
            if (rc) { lep_free(x.outs[i].data); x.outs[i].data = nullptr; x.outs[i].len = x.outs[i].cap = 0; }
        }
        x.status[i] = rc;
        lep_jpeg_close(x.parsed[i]);
        x.parsed[i] = nullptr;
    });
    x.st.write_s += now_s() - t0;
}

// A thread segment that did not fit the stream space reserved for it (sized from its JPEG bytes: the arithmetic coder
// almost never writes more than the Huffman coder did) is not a refusal the reference would make: such files go
// through the per-file path, which reserves the worst case, once the pipeline has drained.
void redo_overflowed(CompressCall& x) {
    for (int i = 0; i < x.n; ++i) {
        if (x.status[i] != LEP_BUFFER_TOO_SMALL) continue;
        lep_bytes o; o.data = nullptr; o.len = o.cap = 0;
        int rc = lep_compress_slice(x.g, x.jpgs[i].data, x.jpgs[i].len, x.start[i], 0, &o);
        if (!rc && x.verify) {   // the arithmetic-coder half of the round-trip check, through the per-file decoder
            lep_bytes back; back.data = nullptr; back.len = back.cap = 0;
            rc = lep_decompress(x.g, o.data, o.len, &back);
            if (!rc && (back.len != x.jpgs[i].len - x.start[i] || memcmp(back.data, x.jpgs[i].data + x.start[i], back.len))) rc = LEP_ROUNDTRIP_FAILURE;
            lep_free(back.data);
            if (rc) { lep_free(o.data); o.data = nullptr; o.len = o.cap = 0; }
        }
        x.outs[i] = o;
        x.status[i] = rc;
        x.st.redone_files += 1;
    }
}

// frame sizes from the SOF markers -> the whole batch is cut into chunks before anything is decoded (lep_batch_plan), so that every image
// can be Huffman-decoded straight into its place in a staging buffer (no page faults, no second copy)
int cut_compress_chunks(CompressCall& x, const lep_batch_options* o, std::vector<std::unique_ptr<Chunk>>* chunks) {
    const int n = x.n;
    std::vector<size_t> fbytes(n, 0), jbytes(n, 0);
    parallel_for(n, x.threads, [&](int i) {
        jbytes[i] = x.jpgs[i].len;
        if (x.start[i] > 0xffffffffu) { x.status[i] = LEP_ASSERTION_FAILURE; return; }   // (lep_jpeg_open_slice's first refusal)
        if (int rc = lep_jpeg_peek_frame_bytes(x.jpgs[i].data, x.jpgs[i].len, &fbytes[i])) { x.status[i] = rc; fbytes[i] = 0; }
    });
    std::vector<int> first((size_t)n + 2, 0);
    const int nchunks = lep_batch_plan(jbytes.data(), fbytes.data(), n, o, first.data(), n + 2);
    if (nchunks < 0) return LEP_ASSERTION_FAILURE;
    for (int k = 0; k < nchunks; ++k) {
        std::unique_ptr<Chunk> c(new Chunk);
        c->first = first[k];
        size_t bytes = 0;
        for (int i = first[k]; i < first[k + 1]; ++i) {
            if (x.status[i]) continue;
            c->live.push_back(i); c->frame_off.push_back(bytes);
            bytes += lepbuf::round_up(fbytes[i]);
        }
        c->count = first[k + 1] - first[k];
        c->frame_bytes = bytes;
        chunks->push_back(std::move(c));
    }
    return 0;
}

}  // namespace

extern "C" {

uint64_t lep_batch_scan_second_chances(void) { return g_scan_second_chances.load(std::memory_order_relaxed); }

// frees the pinned / device staging buffers the batch calls keep between invocations
void lep_batch_release(void) { for (Slot& s : g_slots) s.release(); }

// what the batch calls keep between invocations: bytes of pinned host memory, and of device memory in the large arenas
// (frames, scratch frames, stream / scan arenas, row records; the per-segment tables are KBs and not counted)
void lep_batch_footprint(size_t* pinned_bytes, size_t* device_bytes) {
    size_t pinned = 0, device = 0;
    for (const Slot& s : g_slots) {
#define X(kind, T, name, counted) if (counted) (s.name.pinned ? pinned : device) += s.name.cap;
        LEP_SLOT_BUFFERS(X)
#undef X
    }
    if (pinned_bytes) *pinned_bytes = pinned;
    if (device_bytes) *device_bytes = device;
}

// test hook: fills every pinned staging buffer the batch calls keep between invocations with `value`, so that a test can
// show that nothing stale from an earlier batch (the padding between frames, the tails of streams) reaches a result
void lep_batch_debug_poison(int value) {
    for (Slot& s : g_slots) {
#define X(kind, T, name, counted) if (s.name.pinned && s.name.p) memset(s.name.p, value, s.name.cap);
        LEP_SLOT_BUFFERS(X)
#undef X
    }
}

// test hooks: the check kernels of `verify` on buffers the caller gives, through the launchers launch_compress_chunk uses
int lep_batch_debug_compare(lep_gpu* g, const void* d_a, const void* d_b, size_t bytes, uint32_t* d_flag, uint32_t value) {
    if (!g || !d_flag) return LEP_GPU_ERROR;
    if (((uintptr_t)d_a | (uintptr_t)d_b) % 16 || (uintptr_t)d_flag % 4 || (bytes >= 16 && (!d_a || !d_b))) return LEP_ASSERTION_FAILURE;
    HIPOK(hipSetDevice(lep_gpu_device(g)));
    launch_compare(d_a, d_b, bytes, d_flag, value, nullptr);
    HIPOK(hipGetLastError());
    HIPOK(hipDeviceSynchronize());
    return 0;
}
int lep_batch_debug_scan_check(lep_gpu* g, int bytes_form, const uint8_t* d_out, const uint32_t* d_out_len, const uint8_t* d_ref,
                               const lep_scan_check* items, int n, uint32_t* d_flags) {
    if (!g || n < 0) return LEP_GPU_ERROR;
    if (n == 0) return 0;
    if (!d_out || !d_out_len || !d_ref || !items || !d_flags) return LEP_GPU_ERROR;
    for (int i = 0; i < n; ++i) {
        if (bytes_form ? (items[i].image & kScanCheckPrefix) != 0
                       : (((uintptr_t)d_out + items[i].out_off) | ((uintptr_t)d_ref + items[i].ref_off)) % 16 != 0) return LEP_ASSERTION_FAILURE;
    }
    HIPOK(hipSetDevice(lep_gpu_device(g)));
    lepbuf::DevBuf<ScanCheck> d_items;
    HIPOK(d_items.ensure((size_t)n * sizeof(ScanCheck)));
    hipError_t e = hipMemcpy(d_items, items, (size_t)n * sizeof(ScanCheck), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        (bytes_form ? launch_scan_check_bytes : launch_scan_check)(d_out, d_out_len, d_ref, d_items, (unsigned)n, d_flags, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)d_items.release();
    return e == hipSuccess ? 0 : LEP_GPU_ERROR;
}

// test hook: one alteration for the next compress call (see the header); a new arming forgets the last one's count
void lep_batch_debug_tamper(int where, int file, uint64_t offset, int xor_mask) {
    g_tamper = Tamper();
    if (where < LEP_TAMPER_STREAM || where > LEP_TAMPER_PSCAN || file < 0) return;
    g_tamper.armed = true;
    g_tamper.where = where; g_tamper.file = file; g_tamper.offset = offset; g_tamper.mask = xor_mask;
}
int lep_batch_debug_tamper_applied(void) { return g_tamper.applied; }
int lep_batch_debug_tamper_seen(uint32_t* flags, int32_t* decode_status) {
    if (flags) *flags = g_tamper.seen_flags;
    if (decode_status) *decode_status = g_tamper.seen_status;
    return g_tamper.applied;
}

int lep_compress_batch(lep_gpu* g, const lep_bytes* jpgs, int n, lep_bytes* outs, int32_t* status, const lep_batch_options* o,
                       lep_batch_stats* stats) {
    return lep_compress_batch_slices(g, jpgs, nullptr, n, outs, status, o, stats);
}

// slices[i] = {start_byte, trunc} of files[i] (`lepton -startbyte -trunc`; NULL: whole files): -trunc bounds the reader, so everything
// below sees the file as its first `trunc` bytes; start_byte travels to the parsers, which drop the hand-off rows in front of it, and to
// whatever holds the result against the input -- bytes [start_byte, len).
int lep_compress_batch_slices(lep_gpu* g, const lep_bytes* files, const lep_slice* slices, int n, lep_bytes* outs, int32_t* status,
                              const lep_batch_options* o, lep_batch_stats* stats) {
    struct Disarm { ~Disarm() { g_tamper.armed = false; } } disarm;   // (test hook: an armed alteration is this call's, applied or not)
    if (!g || n < 0) return LEP_GPU_ERROR;
    g_batch_gpu = g;
    std::vector<lep_bytes> bounded(files, files + n);
    std::vector<size_t> start((size_t)n, 0);
    if (slices)
        for (int i = 0; i < n; ++i) {
            if (slices[i].trunc && slices[i].trunc < bounded[i].len) bounded[i].len = slices[i].trunc;
            start[i] = slices[i].start_byte;
        }
    CompressCall x(n);
    x.g = g; x.outs = outs; x.status = status; x.jpgs = bounded.data(); x.start = start.data();
    x.threads = o && o->host_threads > 0 ? o->host_threads : effective_cpus();
    // With the Huffman decode on the GPU, chunk k+1 is decoded (lep_huffdec_simt.h, one lane per piece of the scan, on its own stream)
    // WHILE the split-phase encoder's kernels of chunk k run.  The chunking itself is lep_batch_plan (lep_api.cc).
    x.verify = o && o->verify;
    x.gpu_huffman = !(o && o->host_huffman);
    x.cut_progressive = lep_gpu_cut_progressive(g, -1) != 0;
    HIPOK(hipSetDevice(lep_gpu_device(g)));
    tune_malloc_for_pool();
    const double t_begin = now_s();
    for (int i = 0; i < n; ++i) { outs[i].data = nullptr; outs[i].len = outs[i].cap = 0; status[i] = 0; }
    std::vector<std::unique_ptr<Chunk>> chunks;
    if (int rc = cut_compress_chunks(x, o, &chunks)) return rc;
    // overlap_launches: chunk k+1's coder kernel goes to a second stream (and the library's second workspace set), so its
    // wavefronts start in the slots that chunk k's long thread segments leave free instead of waiting for the last of them
    // (real photographs: segments of equal compressed size differ several-fold in blocks).  Off by default until measured.
    x.overlap = (o && o->overlap_launches) || (getenv("LEP_BATCH_OVERLAP") && atoi(getenv("LEP_BATCH_OVERLAP")) != 0);
    x.streams.g = g;
    if (x.streams.make(&x.s_copy) || x.streams.make(&x.s_compute[0]) || (x.overlap && x.streams.make(&x.s_compute[1])) || x.streams.make(&x.s_down)) return LEP_GPU_ERROR;
    {   // Huffman decode of chunk k+1 beside the coder kernels of chunk k: its workgroups go first whenever a slot is free
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (x.streams.make(&x.s_huff, hi, true)) return LEP_GPU_ERROR;
    }
    Slot* slots = g_slots;   // grow-only staging cache shared by the batch calls (lep_batch_release frees it)
    g_alloc_s = 0;
    int rc_all = 0;
    Joiner writer_guard;   // writes chunk k-1's containers while chunk k is on the GPU
    std::thread& writer = writer_guard.t;
    int slot_i = 0;
    const double t_pipe = now_s();
    if (!chunks.empty()) {
        if (int rc = parse_and_upload(x, chunks[0].get(), &slots[0])) rc_all = rc;
        else if (int rc2 = launch_compress_chunk(x, chunks[0].get(), &slots[0])) rc_all = rc2;
    }
    for (size_t ci = 0; !rc_all && ci < chunks.size(); ++ci, slot_i ^= 1) {
        Slot* s = &slots[slot_i];
        Chunk* c = chunks[ci].get();
        // while this chunk's coder kernels run: Huffman-decode the next chunk into the other slot (its previous user has been
        // written out), beside them on the GPU, and queue ITS coder kernels right behind -- only then fetch this chunk's results,
        // so that the download and the container writing hide under the next chunk's kernels
        if (writer.joinable()) writer.join();
        if (ci + 1 < chunks.size()) {
            if (int rc = parse_and_upload(x, chunks[ci + 1].get(), &slots[slot_i ^ 1])) { rc_all = rc; break; }
            if (int rc = launch_compress_chunk(x, chunks[ci + 1].get(), &slots[slot_i ^ 1])) { rc_all = rc; break; }
        }
        CompressResults r;
        if (int rc = fetch_streams(x, c, s, &r)) { rc_all = rc; break; }
        writer = std::thread([&x, c, s, r]() { write_containers(x, c, s, r); });
    }
    if (writer.joinable()) writer.join();
    x.st.pipeline_s = now_s() - t_pipe;
    for (int i = 0; i < n; ++i) if (x.parsed[i]) { lep_jpeg_close(x.parsed[i]); x.parsed[i] = nullptr; }
    if (!rc_all) redo_overflowed(x);
    x.st.alloc_s = g_alloc_s;
    x.st.wall_s = now_s() - t_begin;
    if (stats) *stats = x.st;
    return rc_all;
}

}  // extern "C"

// ---- .lep -> JPEG, batch ---------------------------------------------------------------------------------------------
namespace {

struct DecompressCall : BatchCall {
    const lep_bytes* leps = nullptr;
    size_t chunk_budget = 0, chunk_images = 0;
    // Consecutive chunks' decode kernels on TWO streams (and the codec's two workspace sets) where that pays: a launch is over when its
    // longest thread segment is, and while the long segments of a ragged chunk (1080p files beside 4K ones; a chunk that does not fill the
    // chip) run on, the wave slots its short ones have left stand empty -- the next chunk's launch, longest segments first, moves into them
    // instead of waiting behind the whole kernel.  A chunk of equal segments that fills the chip keeps the one-stream order: there is no
    // tail to fill, and its scan encoders would only have to fight the next decode kernel for slots (the LEP_BATCH_SCAN_STREAM finding
    // below).  LEP_BATCH_DEC_OVERLAP=0 | 1 forces never / always.  The decisions are lepbatch::LaunchOrder's.
    int dec_overlap = -1;
    // The scan encoders run behind the decoder on ITS stream.  On a stream of their own (LEP_BATCH_SCAN_STREAM=1) they compete with the
    // next chunk's decode kernel for wave slots it fills completely, finish when it does, and hold the chunk's download back:
    // 1530 against 1774 MB/s (profiles/r06j_*).
    bool scan_separate = false;
    // (No fifth stream: the runtime deals its 8 hardware queues out to streams in turn, the codec holds three streams of its own, and
    // the stream that then SHARES a queue with the compute stream has its work -- the next chunk's upload, say -- run behind the decode
    // kernel: measured, 0.77 s of a 1.9 s call (LEP_BATCH_TRACE).  The second compute stream IS the scan stream of LEP_BATCH_SCAN_STREAM=1.)
    hipStream_t s_copy = nullptr, s_compute[2] = {nullptr, nullptr}, s_down = nullptr;
    lepbatch::LaunchOrder order;
    HandleVector<lep_file, lep_file_close> files;
    std::vector<size_t> fbytes;
    explicit DecompressCall(int n_) : files((size_t)n_), fbytes((size_t)n_, 0) { n = n_; }
    void note(const char* what) const { if (trace) fprintf(stderr, "[batch]   %s (t=%.3f)\n", what, now_s() - t_pipe0); }
};

std::unique_ptr<Chunk> cut_chunk(DecompressCall& x, int first) {
    std::unique_ptr<Chunk> c(new Chunk);
    c->first = first;
    size_t bytes = 0;
    int i = first;
    for (; i < x.n; ++i) {
        if (!x.files[i]) continue;
        const size_t fb = x.fbytes[i];
        if (!c->live.empty() && (bytes + fb > x.chunk_budget || c->live.size() >= x.chunk_images)) break;
        c->live.push_back(i); c->frame_off.push_back(bytes);
        bytes += fb;
    }
    c->count = i - first;
    c->frame_bytes = bytes;
    c->offs.push_back(0);
    return c;
}

// a file the GPU encoders gave back after the launch: the host re-coder reads its frame where the D2H copy puts it, the slot's pinned
// buffer (reserved at the chunk's full size: a buffer that already holds frames of this chunk is large enough and does not move)
int send_to_host_recoder(DecompressCall& x, Chunk* c, Slot* s, size_t k) {
    if (int rc = pinned_reserve(s->h_frames, c->frame_bytes)) return rc;
    lep_file_describe_into(x.files[c->live[k]], s->h_frames + c->frame_off[k], x.fbytes[c->live[k]], &c->host_desc[k]);
    return 0;
}

// stage 1: streams into the slot's pinned arena (packed back to back); geometry of every frame (the frames themselves are decoded into
// device memory)
int stage_streams(DecompressCall& x, Chunk* c, Slot* s, std::vector<uint32_t>* lens) {
    c->segs.clear(); c->offs.assign(1, 0); c->seg_first.clear(); lens->clear();
    std::vector<const uint8_t*> src;
    for (size_t k = 0; k < c->live.size(); ++k) {
        lep_segment sg[LEP_MAX_SEGMENTS];
        lep_bytes sb[LEP_MAX_SEGMENTS];
        const int ns = lep_file_segments(x.files[c->live[k]], sg, sb, (int)k);
        c->seg_first.push_back((int)c->segs.size());
        for (int q = 0; q < ns; ++q) {
            c->segs.push_back(sg[q]);
            lens->push_back((uint32_t)sb[q].len);
            src.push_back(sb[q].data);
            c->offs.push_back(c->offs.back() + sb[q].len);
        }
    }
    c->seg_first.push_back((int)c->segs.size());
    if (int rc = slot_reserve(s, c->frame_bytes, c->offs.back() + 256, c->segs.size(), c->live.size(), false, c->offs.back() + 256)) return rc;
    x.note("slot reserved");
    const double t0 = now_s();
    parallel_for((int)c->segs.size(), x.threads, [&](int q) { if ((*lens)[q]) memcpy(s->h_streams + c->offs[q], src[q], (*lens)[q]); });
    x.note("streams staged");
    x.st.stage_s += now_s() - t0;
    c->host_desc.resize(c->live.size());
    for (size_t k = 0; k < c->live.size(); ++k) lep_file_describe_into(x.files[c->live[k]], nullptr, (size_t)-1, &c->host_desc[k]);
    c->dev_desc = c->host_desc;
    for (size_t k = 0; k < c->live.size(); ++k) point_into_frame(c->dev_desc[k].blocks, c->host_desc[k], s->d_frames + c->frame_off[k]);
    return 0;
}

// stage 2a: GPU Huffman re-encode plan: eligible files get their scan bytes back instead of their frames
void plan_sequential_recode(DecompressCall& x, Chunk* c, Slot* s) {
    auto none = [&]() { c->himg.clear(); c->hseg.clear(); c->hfirst.assign(c->live.size(), -1); c->hslot.clear(); c->hbound.clear(); c->scan_bytes = 0; };
    none();
    if (!x.gpu_huffman) return;
    lepbatch::OutputArena arena;
    for (size_t k = 0; k < c->live.size(); ++k) {
        lep_huff_image hi;
        lep_huff_segment hs[LEP_MAX_SEGMENTS];
        int ns = 0, ok = 0;
        if (lep_file_recode_plan(x.files[c->live[k]], &hi, hs, &ns, &ok) || !ok) continue;
        point_into_frame(hi.blocks, c->host_desc[k], s->d_frames + c->frame_off[k]);
        c->hfirst[k] = (int)c->hseg.size();
        uint32_t caps[LEP_MAX_SEGMENTS];
        lepbatch::RecodeSlot at[LEP_MAX_SEGMENTS];
        for (int q = 0; q < ns; ++q) caps[q] = hs[q].out_cap;
        lepbatch::place_recode_segments(caps, ns, &arena, at);
        for (int q = 0; q < ns; ++q) {
            hs[q].image = (int32_t)c->himg.size();
            hs[q].out_off = at[q].off;
            hs[q].out_cap = at[q].slot;
            c->hslot.push_back(at[q].slot); c->hbound.push_back(at[q].bound);
            c->hseg.push_back(hs[q]);
        }
        c->himg.push_back(hi);
    }
    c->scan_bytes = arena.bytes;
    // no room for the scan arena (hostile hand-off sizes are clamped by recode_prepare, so this is a real shortage):
    // the chunk's files take the host re-coder instead of failing everybody's request
    if (!c->hseg.empty() && scan_reserve(s, c->scan_bytes + 256, c->hseg.size())) none();
}
// stage 2b: progressive files: every scan is a function of the finished frame -> one GPU wavefront per (image, scan)
void plan_progressive_recode(DecompressCall& x, Chunk* c, Slot* s) {
    auto none = [&]() { c->pimg.clear(); c->pscan.clear(); c->pfirst.assign(c->live.size(), -1); c->pcount.assign(c->live.size(), 0); };
    none();
    c->pscan_bytes = 0; c->corr_words = 0;
    if (!x.gpu_huffman) return;
    lepbatch::OutputArena arena;
    std::vector<lep_huffprog_scan> tmp(256);
    for (size_t k = 0; k < c->live.size(); ++k) {
        if (c->hfirst[k] >= 0) continue;
        lep_huffprog_image pi;
        int ns = 0, ok = 0;
        if ((x.cut_progressive ? lep_file_recode_plan_progressive_cut : lep_file_recode_plan_progressive)(x.files[c->live[k]], &pi, tmp.data(), (int)tmp.size(), &ns, &ok) || !ok) continue;
        point_into_frame(pi.blocks, c->host_desc[k], s->d_frames + c->frame_off[k]);
        c->pfirst[k] = (int)c->pscan.size(); c->pcount[k] = ns;
        for (int q = 0; q < ns; ++q) {
            tmp[q].image = (int32_t)c->pimg.size();
            tmp[q].out_off = arena.place(tmp[q].out_cap);
            tmp[q].corr_off = (uint32_t)arena.place_corr(tmp[q].corr_cap);
            c->pscan.push_back(tmp[q]);
        }
        c->pimg.push_back(pi);
    }
    c->pscan_bytes = arena.bytes; c->corr_words = arena.corr_words;
    if (!c->pscan.empty() && (c->corr_words > 0xfffffff0u || prog_reserve(s, c->pscan_bytes + 256, c->corr_words + 16, c->pscan.size()))) none();   // no room: host re-coder
}

// stage 3: upload; frames zeroed on the device where they have to be
int upload_streams(DecompressCall& x, Chunk* c, Slot* s, std::vector<uint32_t>* lens) {
    HIPOK(hipMemcpyAsync(s->d_streams, s->h_streams, c->offs.back(), hipMemcpyHostToDevice, x.s_copy));
    HIPOK(hipMemcpyAsync(s->d_len, lens->data(), lens->size() * 4, hipMemcpyHostToDevice, x.s_copy));
    // The decode kernel stores every coefficient of every block it decodes: only a file whose frame holds blocks that are NOT coded
    // (a truncated one) needs its frame cleared.  (Clearing the whole chunk was a 25 GB fill kernel that could not start while the
    // previous chunk's decoder held every wave slot, and this function waited for it.)
    for (size_t k = 0; k < c->live.size(); ++k) {
        const lep_image_desc& d = c->host_desc[k];
        bool whole = true;
        for (int cc = 0; cc < d.ncomp; ++cc) whole = whole && d.coded_blocks[cc] == d.width_blocks[cc] * d.height_blocks[cc];
        if (!whole) HIPOK(hipMemsetAsync(s->d_frames + c->frame_off[k], 0, x.fbytes[c->live[k]], x.s_copy));
    }
    x.note("copies queued");
    HIPOK(hipEventRecord(s->up, x.s_copy));
    HIPOK(hipStreamSynchronize(x.s_copy));   // `lens` / pinned arena are reused by the caller
    x.st.h2d_bytes += (double)c->offs.back();
    return 0;
}

int stage_and_upload(DecompressCall& x, Chunk* c, Slot* s, std::vector<uint32_t>* lens) {
    if (c->live.empty()) return 0;
    if (x.trace) fprintf(stderr, "[batch] stage_and_upload first=%d begins (t=%.3f)\n", c->first, now_s() - x.t_pipe0);
    if (int rc = stage_streams(x, c, s, lens)) return rc;
    plan_sequential_recode(x, c, s);
    plan_progressive_recode(x, c, s);
    // files the host re-coder handles: the pinned frames are reserved ONCE, before any frame pointer into them is handed out
    bool any_host = false;
    for (size_t k = 0; k < c->live.size(); ++k) { any_host |= c->hfirst[k] < 0 && c->pfirst[k] < 0; if (c->hfirst[k] >= 0 || c->pfirst[k] >= 0) x.st.gpu_huffman_files += 1; }
    if (any_host) {
        if (int rc = pinned_reserve(s->h_frames, c->frame_bytes)) return rc;
        for (size_t k = 0; k < c->live.size(); ++k)
            if (c->hfirst[k] < 0 && c->pfirst[k] < 0) lep_file_describe_into(x.files[c->live[k]], s->h_frames + c->frame_off[k], x.fbytes[c->live[k]], &c->host_desc[k]);
    }
    x.note("plans made");
    if (int rc = upload_streams(x, c, s, lens)) return rc;
    if (x.trace) fprintf(stderr, "[batch] stage_and_upload first=%d done (t=%.3f)\n", c->first, now_s() - x.t_pipe0);
    return 0;
}

// decoder + Huffman re-encode kernels of one chunk: stream-ordered behind the previous chunk's, or beside them on the other stream
// when the previous chunk leaves wave slots to fill (lepbatch::LaunchOrder)
int launch_decompress_chunk(DecompressCall& x, Chunk* c, Slot* s) {
    const int nseg = (int)c->segs.size(), nimg = (int)c->live.size();
    if (!nimg) return 0;
    const double tt0 = now_s();
    // does THIS chunk leave a tail?  the block counts of its thread segments
    int64_t lo = INT64_MAX, hi = 0;
    for (int q = 0; q < nseg; ++q) {
        const lep_image_desc& d = c->dev_desc[(size_t)c->segs[q].image];
        const int y1 = c->segs[q].is_last ? d.height_blocks[0] : std::min<int>(c->segs[q].luma_y_end, d.height_blocks[0]);
        const int64_t w = std::max<int64_t>(1, (int64_t)std::max(0, y1 - c->segs[q].luma_y_start) * d.width_blocks[0]);
        lo = std::min(lo, w); hi = std::max(hi, w);
    }
    const lepbatch::LaunchPlace at = x.order.step(lo, hi, nseg, x.dec_overlap, x.scan_separate, !(c->count < x.n), (int)(s - g_slots));
    hipStream_t s_compute = x.s_compute[at.stream];
    hipStream_t s_scan = x.scan_separate ? x.s_compute[1] : s_compute;
    // this slot's buffers were last used by the chunk before the previous one, possibly on the other stream -- and a workspace set by
    // either of the two chunks in front
    // (At most ONE earlier chunk is in flight when this runs: the caller has fetched -- waited for the download of -- every chunk but
    // the one in front before it launches this one.  A launch that is not `beside` goes onto the previous launch's stream, so stream
    // order is its dependency; ADVICE round 5: the extra wait that stood here could never fire.)
    if (s->done_recorded) HIPOK(hipStreamWaitEvent(s_compute, s->done, 0));
    HIPOK(hipStreamWaitEvent(s_compute, s->up, 0));
    if (int rc0 = lep_gpu_use_arena(x.g, at.set)) return rc0;
    (void)lep_gpu_expect_company(x.g, at.expect_company);
    int rc = lep_gpu_decode_device(x.g, c->dev_desc.data(), nimg, c->segs.data(), nseg, s->d_streams, c->offs.data(), s->d_len, s->d_status, s_compute);
    (void)lep_gpu_expect_company(x.g, 0);
    (void)lep_gpu_use_arena(x.g, 0);
    if (rc) return rc;
    // A progressive file that ends inside a scan and was coded as ONE thread segment: the reference's re-coder reads zeros for every block at
    // or behind trunc_bc -- even where the stream codes the first block of a later row (recode_progressive's lazy_tail).  The scan writers
    // get the same view: those blocks are cleared behind the decode, in front of the scan launch.  Several segments: the frame as it is.
    for (size_t k = 0; k < c->live.size(); ++k) {
        if (c->pfirst[k] < 0 || c->seg_first[k + 1] - c->seg_first[k] != 1) continue;
        const lep_image_desc& d = c->host_desc[k];
        for (int cc = 0; cc < d.ncomp; ++cc) {
            const int64_t all = (int64_t)d.width_blocks[cc] * d.height_blocks[cc], coded = d.coded_blocks[cc];
            if (coded >= 0 && coded < all) HIPOK(hipMemsetAsync(c->dev_desc[k].blocks[cc] + coded * 64, 0, (size_t)(all - coded) * 128, s_compute));
        }
    }
    // NOT redundant: the scan encoders' descriptors live in ONE device buffer of the codec, whichever workspace set the decoder used (the
    // encoders always take set 0's).  A launch beside the previous one is on the other stream, so nothing else orders this chunk's
    // descriptor upload behind the previous chunk's encoders, which still read that buffer: this wait on the previous slot's `done` is
    // what keeps overlapped chunks from sharing set 0's encoder descriptors.
    if (at.beside && at.prev_slot >= 0 && g_slots[at.prev_slot].done_recorded) HIPOK(hipStreamWaitEvent(s_scan, g_slots[at.prev_slot].done, 0));
    const double tt1 = now_s();
    if (s_scan != s_compute) { HIPOK(hipEventRecord(s->decoded, s_compute)); HIPOK(hipStreamWaitEvent(s_scan, s->decoded, 0)); }
    if (!c->hseg.empty()) {
        rc = lep_gpu_huffman_encode_device(x.g, c->himg.data(), (int)c->himg.size(), c->hseg.data(), (int)c->hseg.size(), s->d_scan, s->d_scanlen, huff_ends(s, c->hseg.size()), s_scan);
        if (rc) return rc;
    }
    if (x.trace) fprintf(stderr, "[batch] launch_chunk first=%d: decode launch %.3f s, scan-encode launch %.3f s (t=%.3f)\n", c->first, tt1 - tt0, now_s() - tt1, now_s() - x.t_pipe0);
    if (!c->pscan.empty()) {
        rc = lep_gpu_huffman_progressive_encode_device(x.g, c->pimg.data(), (int)c->pimg.size(), c->pscan.data(), (int)c->pscan.size(), s->d_pscan, s->d_corr,
                                                       s->d_pscanlen, s_scan);
        if (rc) return rc;
    }
    HIPOK(hipEventRecord(s->done, s_scan));
    s->done_recorded = true;
    return 0;
}

struct DecompressResults {   // a chunk's results as fetched: copied by value into the writer thread
    std::vector<int32_t> sts;                  // per segment: decoder statuses
    std::vector<uint32_t> slens, plens;        // per hseg / per pscan: bytes written
    std::vector<lep_huff_end> sends;           // per hseg: end states
    std::vector<size_t> poff;                  // packed offsets of the progressive scans in the pinned mirror
};

// the progressive scans come down packed; a file with a scan that outgrew its slot or its scratch takes the host re-coder
int fetch_progressive_scans(DecompressCall& x, Chunk* c, Slot* s, DecompressResults* r) {
    const int nimg = (int)c->live.size();
    lepbatch::OutputArena packed;
    for (int k = 0; k < nimg; ++k) {
        if (c->pfirst[k] < 0) continue;
        bool fits = true;
        for (int q = c->pfirst[k]; q < c->pfirst[k] + c->pcount[k]; ++q) fits = fits && !(r->plens[q] & 0x80000000u);
        if (!fits) {
            c->pfirst[k] = -1;
            if (int rc = send_to_host_recoder(x, c, s, (size_t)k)) return rc;
            continue;
        }
        for (int q = c->pfirst[k]; q < c->pfirst[k] + c->pcount[k]; ++q) r->poff[q] = packed.place(r->plens[q]);
    }
    if (int rc = pinned_reserve(s->h_pscan, packed.bytes + 256, (packed.bytes + 256) / 4)) return rc;
    for (int k = 0; k < nimg; ++k) {
        if (c->pfirst[k] < 0) continue;
        for (int q = c->pfirst[k]; q < c->pfirst[k] + c->pcount[k]; ++q)
            if (r->plens[q]) { HIPOK(hipMemcpyAsync(s->h_pscan + r->poff[q], s->d_pscan + c->pscan[q].out_off, r->plens[q], hipMemcpyDeviceToHost, x.s_down)); x.st.d2h_bytes += r->plens[q]; }
    }
    return 0;
}

// The scan bytes of the GPU-coded files come down in one copy of the arena range they lie in (same reasoning as the compressor's
// streams: 8195 copies per chunk took 370 ms), unless that range is mostly slack; a file whose answer does not stand
// (lepbatch::gpu_answer_stands) and the files the GPU encoders never took get their frames down for the host re-coder
int fetch_sequential_scans(DecompressCall& x, Chunk* c, Slot* s, DecompressResults* r) {
    const int nimg = (int)c->live.size();
    const std::vector<uint32_t>& slens = r->slens;
    std::vector<char> stands(nimg, 0);
    size_t scan_lo = ~(size_t)0, scan_hi = 0, scan_live = 0;
    for (int k = 0; k < nimg; ++k) {
        if (c->pfirst[k] >= 0 || c->hfirst[k] < 0) continue;
        const int h0 = c->hfirst[k], h1 = h0 + (c->seg_first[k + 1] - c->seg_first[k]);
        stands[k] = lepbatch::gpu_answer_stands(slens.data() + h0, c->hslot.data() + h0, c->hbound.data() + h0, r->sends.data() + h0, h1 - h0);
        if (!stands[k]) continue;
        for (int q = h0; q < h1; ++q) if (slens[q]) {
            scan_lo = std::min<size_t>(scan_lo, c->hseg[q].out_off); scan_hi = std::max<size_t>(scan_hi, (size_t)c->hseg[q].out_off + slens[q]);
            scan_live += slens[q];
        }
    }
    const bool scan_whole = scan_hi > scan_lo && lepbatch::download_whole(scan_hi - scan_lo, scan_live);
    if (scan_whole) {
        HIPOK(hipMemcpyAsync(s->h_scan + scan_lo, s->d_scan + scan_lo, scan_hi - scan_lo, hipMemcpyDeviceToHost, x.s_down));
        x.st.d2h_bytes += (double)(scan_hi - scan_lo);
    }
    int rc_late = 0;
    for (int k = 0; k < nimg; ++k) {
        if (c->pfirst[k] >= 0) continue;
        if (c->hfirst[k] >= 0 && !stands[k]) {   // a segment that filled its reserved slot may have been cut short: let the host redo that file
            x.st.gpu_huffman_files -= 1;
            c->hfirst[k] = -1;
            if ((rc_late = send_to_host_recoder(x, c, s, (size_t)k))) break;
        }
        if (c->hfirst[k] >= 0) {
            const int h0 = c->hfirst[k], h1 = h0 + (c->seg_first[k + 1] - c->seg_first[k]);
            if (!scan_whole) for (int q = h0; q < h1; ++q)
                if (slens[q]) { HIPOK(hipMemcpyAsync(s->h_scan + c->hseg[q].out_off, s->d_scan + c->hseg[q].out_off, slens[q], hipMemcpyDeviceToHost, x.s_down)); x.st.d2h_bytes += slens[q]; }
        } else {
            const size_t fb = (k + 1 < nimg ? c->frame_off[k + 1] : c->frame_bytes) - c->frame_off[k];
            HIPOK(hipMemcpyAsync(s->h_frames + c->frame_off[k], s->d_frames + c->frame_off[k], fb, hipMemcpyDeviceToHost, x.s_down));
            x.st.d2h_bytes += (double)fb;
        }
    }
    HIPOK(hipStreamSynchronize(x.s_down));
    return rc_late;
}

int fetch_scans(DecompressCall& x, Chunk* c, Slot* s, DecompressResults* r) {
    const int nseg = (int)c->segs.size(), nimg = (int)c->live.size();
    r->sts.assign(nseg, 0); r->slens.assign(c->hseg.size(), 0); r->plens.assign(c->pscan.size(), 0);
    r->sends.assign(c->hseg.size(), lep_huff_end()); r->poff.assign(c->pscan.size(), 0);
    if (!nimg) return 0;
    HIPOK(hipStreamWaitEvent(x.s_down, s->done, 0));
    HIPOK(hipMemcpyAsync(r->sts.data(), s->d_status, (size_t)nseg * 4, hipMemcpyDeviceToHost, x.s_down));
    if (!c->hseg.empty()) HIPOK(hipMemcpyAsync(r->slens.data(), s->d_scanlen, c->hseg.size() * 4, hipMemcpyDeviceToHost, x.s_down));
    if (!c->hseg.empty()) HIPOK(hipMemcpyAsync(r->sends.data(), huff_ends(s, c->hseg.size()), c->hseg.size() * sizeof(lep_huff_end), hipMemcpyDeviceToHost, x.s_down));
    if (!c->pscan.empty()) HIPOK(hipMemcpyAsync(r->plens.data(), s->d_pscanlen, c->pscan.size() * 4, hipMemcpyDeviceToHost, x.s_down));
    HIPOK(hipStreamSynchronize(x.s_down));
    if (!c->pscan.empty()) { if (int rc = fetch_progressive_scans(x, c, s, r)) return rc; }
    return fetch_sequential_scans(x, c, s, r);
}

// JPEG files on the host pool (the writer thread)
void write_jpegs(DecompressCall& x, Chunk* c, Slot* s, const DecompressResults& r) {
    const double t0 = now_s();
    parallel_for((int)c->live.size(), x.threads, [&](int k) {
        const int i = c->live[k];
        int rc = 0;
        for (int q = c->seg_first[k]; q < c->seg_first[k + 1]; ++q) if (r.sts[q] && !rc) rc = r.sts[q];
        if (!rc && c->hfirst[k] >= 0) {   // GPU-coded scan bytes: glue header, segments, trailer
            const int h0 = c->hfirst[k], ns = c->seg_first[k + 1] - c->seg_first[k];
            lep_bytes sb[LEP_MAX_SEGMENTS];
            for (int q = 0; q < ns; ++q) { sb[q].data = s->h_scan + c->hseg[h0 + q].out_off; sb[q].len = sb[q].cap = r.slens[h0 + q]; }
            rc = lep_file_recode_finish(x.files[i], sb, r.sends.data() + h0, ns, &x.outs[i]);
        } else if (!rc && c->pfirst[k] >= 0) {   // progressive file, scans coded on the GPU: glue header pieces and scans
            const int p0 = c->pfirst[k], ns = c->pcount[k];
            std::vector<lep_bytes> sb((size_t)ns);
            for (int q = 0; q < ns; ++q) { sb[q].data = s->h_pscan + r.poff[p0 + q]; sb[q].len = sb[q].cap = r.plens[p0 + q]; }
            rc = lep_file_recode_finish_progressive(x.files[i], sb.data(), ns, &x.outs[i]);
        } else if (!rc) rc = lep_file_recode(x.files[i], &x.outs[i]);   // host re-coder reads the frame in place (pinned D2H buffer)
        x.status[i] = rc;
        lep_file_close(x.files[i]);
        x.files[i] = nullptr;
    });
    x.st.write_s += now_s() - t0;
}

}  // namespace

extern "C" int lep_decompress_batch(lep_gpu* g, const lep_bytes* leps, int n, lep_bytes* outs, int32_t* status, const lep_batch_options* o,
                                    lep_batch_stats* stats) {
    if (!g || n < 0) return LEP_GPU_ERROR;
    g_batch_gpu = g;
    DecompressCall x(n);
    x.g = g; x.outs = outs; x.status = status; x.leps = leps;
    x.threads = o && o->host_threads > 0 ? o->host_threads : effective_cpus();
    x.chunk_budget = o && o->chunk_frame_bytes ? o->chunk_frame_bytes : ((size_t)32 << 30);
    x.chunk_images = o && o->chunk_images > 0 ? (size_t)o->chunk_images : 1024;
    x.gpu_huffman = !(o && o->host_huffman);
    x.cut_progressive = lep_gpu_cut_progressive(g, -1) != 0;
    HIPOK(hipSetDevice(lep_gpu_device(g)));
    tune_malloc_for_pool();
    const double t_begin = now_s();
    for (int i = 0; i < n; ++i) { outs[i].data = nullptr; outs[i].len = outs[i].cap = 0; status[i] = 0; }
    std::vector<char> chained(n, 0);
    {
        const double t0 = now_s();
        parallel_for(n, x.threads, [&](int i) {
            int rc = lep_file_open(leps[i].data, leps[i].len, &x.files[i]);
            if (!rc && lep_chained_file_follows(leps[i].data, leps[i].len, lep_file_consumed(x.files[i]))) {
                chained[i] = 1;   // a stream of several v2+ files: the per-file path walks it once the pipeline has drained
                lep_file_close(x.files[i]); x.files[i] = nullptr;
                return;
            }
            if (!rc) x.fbytes[i] = lepbuf::round_up(lep_file_frame_bytes(x.files[i]));
            if (rc) { status[i] = rc; if (x.files[i]) { lep_file_close(x.files[i]); x.files[i] = nullptr; } }
        });
        x.st.parse_s += now_s() - t0;
    }
    x.streams.g = g;
    if (x.streams.make(&x.s_copy) || x.streams.make(&x.s_compute[0]) || x.streams.make(&x.s_down) || x.streams.make(&x.s_compute[1])) return LEP_GPU_ERROR;
    if (const char* e = getenv("LEP_BATCH_DEC_OVERLAP")) x.dec_overlap = atoi(e) ? 1 : 0;
    x.scan_separate = getenv("LEP_BATCH_SCAN_STREAM") && atoi(getenv("LEP_BATCH_SCAN_STREAM")) == 1;
    Slot* slots = g_slots;
    g_alloc_s = 0;
    int rc_all = 0;
    std::vector<std::vector<uint32_t>> chunk_lens(2);
    x.t_pipe0 = now_s();
    Joiner writer_guard;
    std::thread& writer = writer_guard.t;
    for (int k = 0; k < 2; ++k) slots[k].done_recorded = false;   // (events of an earlier call: nothing of it is in flight)
    std::unique_ptr<Chunk> cur = cut_chunk(x, 0), nxt;
    int slot_i = 0;
    if (int rc = stage_and_upload(x, cur.get(), &slots[0], &chunk_lens[0])) rc_all = rc;
    const double t_pipe = now_s();
    // A host-to-device copy does not run beside a decode kernel on this platform (kernel + copy traces of rounds 4 and 5: the copies sit in
    // the gaps between the kernels; LEP_BATCH_TRACE: the upload of chunk k + 1 returns when chunk k's kernel ends).  For chunks of equal
    // segments that costs nothing -- the next kernel could not start earlier anyway.  But the SECOND chunk of a ragged call is what should
    // move into the wave slots the first one's short segments leave: so when the first chunk is ragged, the second is staged and uploaded
    // BEFORE the first is launched, and both launches go out back to back (the second beside the first: lepbatch::LaunchOrder).  Behind a
    // chunk of equal segments the second launch waits in stream order as before, and only saves its upload's place in the gap (~30 ms).
    bool second_is_staged = false;
    if (!rc_all && cur && cur->count > 0 && x.dec_overlap != 0 && !x.scan_separate && cur->first + cur->count < n) {
        nxt = cut_chunk(x, cur->first + cur->count);
        if (int rc = stage_and_upload(x, nxt.get(), &slots[1], &chunk_lens[1])) rc_all = rc;
        second_is_staged = true;
    }
    if (!rc_all && cur && cur->count > 0) rc_all = launch_decompress_chunk(x, cur.get(), &slots[0]);
    if (!rc_all && second_is_staged && nxt && nxt->count > 0) rc_all = launch_decompress_chunk(x, nxt.get(), &slots[1]);
    while (!rc_all && cur && cur->count > 0) {
        Slot* s = &slots[slot_i];
        // stage the next chunk and queue its kernels behind this chunk's before fetching this chunk's results
        if (writer.joinable()) writer.join();
        if (second_is_staged) second_is_staged = false;   // (the call's second chunk: staged and launched above)
        else {
            nxt = cur->first + cur->count < n ? cut_chunk(x, cur->first + cur->count) : nullptr;
            if (nxt) {
                if (int rc = stage_and_upload(x, nxt.get(), &slots[slot_i ^ 1], &chunk_lens[slot_i ^ 1])) { rc_all = rc; break; }
                if (nxt->count > 0) { if (int rc = launch_decompress_chunk(x, nxt.get(), &slots[slot_i ^ 1])) { rc_all = rc; break; } }
            }
        }
        DecompressResults r;
        if (int rc = fetch_scans(x, cur.get(), s, &r)) { rc_all = rc; break; }
        std::shared_ptr<Chunk> keep(cur.release());
        writer = std::thread([&x, keep, s, r]() { write_jpegs(x, keep.get(), s, r); });
        cur = std::move(nxt);
        slot_i ^= 1;
    }
    if (writer.joinable()) writer.join();
    x.st.pipeline_s = now_s() - t_pipe;
    for (int i = 0; i < n; ++i) if (x.files[i]) { lep_file_close(x.files[i]); x.files[i] = nullptr; }
    if (!rc_all)
        for (int i = 0; i < n; ++i)
            if (chained[i]) status[i] = lep_decompress(g, leps[i].data, leps[i].len, &outs[i]);
    x.st.alloc_s = g_alloc_s;
    x.st.wall_s = now_s() - t_begin;
    if (stats) *stats = x.st;
    return rc_all;
}
