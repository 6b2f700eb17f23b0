// serve_stream_stress.cc -- thread-safety harness for the piecewise answers of lep_serve.cc (stream_band_mcu_rows): built with
// -fsanitize=thread from this file and lep_serve.cc alone, run as a program of its own.  A C stream_process sinks a few hundred small
// pieces for every connection of its batch, a short pause after every round, while eight clients read them as they come; one client in
// four hangs up part-way.  Every complete answer must be the pieces in order.  Exit code 0 and a silent sanitizer = pass.
//   usage: serve_stream_stress <socket path> <rounds>
#include <sys/socket.h>
#include <sys/un.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/lepton_mi355x.h"

// the batch entry points lep_serve.cc references; never reached (the harness installs its own processors)
extern "C" int lep_compress_batch(lep_gpu*, const lep_bytes*, int, lep_bytes*, int32_t*, const lep_batch_options*, lep_batch_stats*) { return LEP_GPU_ERROR; }
extern "C" int lep_decompress_batch(lep_gpu*, const lep_bytes*, int, lep_bytes*, int32_t*, const lep_batch_options*, lep_batch_stats*) { return LEP_GPU_ERROR; }

static const int kPieces = 300;
static std::atomic<long> g_calls{0}, g_gone{0};

static size_t piece_of(uint8_t tag, int k, uint8_t* out) {   // piece k of the file tagged `tag`: 1 .. 97 bytes
    const size_t n = 1 + (size_t)((k * 37 + tag) % 97);
    for (size_t i = 0; i < n; ++i) out[i] = (uint8_t)(tag + k + i);
    return n;
}

// round-robin over the files, like bands of a session; a file whose sink said "gone" gets nothing more and fails
static int stream_process(void*, const lep_bytes* in, int n, lep_batch_sink sink, void* sink_user, int32_t* status) {
    ++g_calls;
    std::vector<char> gone((size_t)n, 0);
    uint8_t buf[128];
    for (int k = 0; k < kPieces; ++k) {
        for (int i = 0; i < n; ++i) {
            if (gone[(size_t)i]) continue;
            const size_t len = piece_of(in[i].data[2], k, buf);
            if (sink(sink_user, i, buf, len)) { gone[(size_t)i] = 1; ++g_gone; }
        }
        if (k % 8 == 0) std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    for (int i = 0; i < n; ++i) status[i] = gone[(size_t)i] ? LEP_OS_ERROR : 0;
    return 0;
}

static int dial(const char* path) {
    const int fd = socket(AF_UNIX, SOCK_STREAM, 0);
    sockaddr_un a;
    memset(&a, 0, sizeof a);
    a.sun_family = AF_UNIX;
    strncpy(a.sun_path, path, sizeof a.sun_path - 1);
    if (connect(fd, reinterpret_cast<sockaddr*>(&a), sizeof a) != 0) { close(fd); return -1; }
    return fd;
}

static std::atomic<long> g_ok{0}, g_bad{0}, g_left{0};

static void client(const char* path, unsigned id, int rounds) {
    for (int r = 0; r < rounds; ++r) {
        const uint8_t tag = (uint8_t)(id * 16 + r);
        const bool leaves = (id + (unsigned)r) % 4 == 3;
        const uint8_t msg[4] = {0xcf, 0x84, tag, 0};
        const int fd = dial(path);
        if (fd < 0) { ++g_bad; continue; }
        if (send(fd, msg, sizeof msg, MSG_NOSIGNAL) != (ssize_t)sizeof msg) { close(fd); ++g_bad; continue; }
        shutdown(fd, SHUT_WR);
        std::vector<uint8_t> ans, want;
        uint8_t buf[4096];
        for (int k = 0; k < kPieces; ++k) { const size_t n = piece_of(tag, k, buf); want.insert(want.end(), buf, buf + n); }
        for (;;) {
            const ssize_t got = recv(fd, buf, sizeof buf, 0);
            if (got <= 0) break;
            ans.insert(ans.end(), buf, buf + got);
            if (leaves && ans.size() > want.size() / 3) break;
        }
        close(fd);
        if (leaves) { ++g_left; if (ans.size() > want.size() || memcmp(ans.data(), want.data(), ans.size())) ++g_bad; continue; }
        ans == want ? ++g_ok : ++g_bad;
    }
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const char* path = argv[1];
    const int rounds = atoi(argv[2]);
    lep_serve_options o;
    memset(&o, 0, sizeof o);
    o.uds_path = path;
    o.max_batch = 8;
    o.batch_window_us = 3000;
    o.stream_band_mcu_rows = 1;
    o.stream_process = stream_process;
    lep_server* srv = nullptr;
    if (lep_serve_start(&o, &srv) != 0) { fprintf(stderr, "cannot start\n"); return 3; }
    std::vector<std::thread> ts;
    for (unsigned i = 0; i < 8; ++i) ts.emplace_back(client, path, i, rounds);
    for (auto& t : ts) t.join();
    lep_serve_stats st;
    for (int k = 0; k < 2000; ++k) {   // the last hang-ups are counted when the IO thread has seen them
        lep_serve_get_stats(srv, &st);
        if (st.answered + st.failed + st.timed_out >= st.accepted) break;
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    lep_serve_stop(srv);
    fprintf(stderr, "clients: %ld whole answers, %ld wrong, %ld left early; server: %llu accepted, %llu answered, %llu in pieces, %llu failed, %llu bytes out before done, %ld calls, %ld sinks refused\n",
            g_ok.load(), g_bad.load(), g_left.load(), (unsigned long long)st.accepted, (unsigned long long)st.answered, (unsigned long long)st.streamed,
            (unsigned long long)st.failed, (unsigned long long)st.bytes_out_before_done, g_calls.load(), g_gone.load());
    return g_bad.load() == 0 && g_ok.load() > 0 && st.streamed == (unsigned long long)g_ok.load() ? 0 : 1;
}
