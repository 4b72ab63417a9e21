// state_rows.hip.h - per-stream save / restore / zero of the engine's carried state (se_realtime_process_chains).
//
// Every state tensor of the engine is STREAM-major: the conv history of encoder level i is row b of one ring slot of xinP[i]
// ([slot][b][C8][PL][T][F] 16-byte pieces), the preconv history row b of a pinP[i] slot (or of pin[i][parity], fp32), the GRU state of
// layer l row b of hbuf[l][hcur] (H floats).  So "the state of stream b" is one contiguous row per tensor, and moving the state of a
// set of streams is a gather / scatter of whole rows:
//   zero     the rows of the streams a call resets (flag = 0 among continuing streams): src = nullptr
//   save     live tensor -> carry buffer of the same row layout, right after the stage work of the segment that is the stream's last
//   restore  carry buffer -> live tensor at call exit, for every stream that ended before the longest one
// One launch moves every tensor of the table for every listed stream: blockIdx.z = table entry, blockIdx.y = position in the stream
// list, blockIdx.x strides over the row.  Pure bandwidth: 16-byte loads and plain 16-byte vector stores when the row is a whole number
// of 16-byte pieces (always for the plane tensors; fp32 rows of odd sizes move word by word), no atomics, no reductions; a row's bytes
// depend on nothing but that row, so results do not depend on the batch or on launch order.
//
// WHERE stream b's state lives is written once per engine: an enumerator of (live tensor, carry buffer, words per stream row) - state_rows_of
// in se_engine.hip, fsn_state_rows_of in fsn_engine.inc.h.  The chain save / restore / zero (through a StateRowList below), the carry
// allocation and *_reset_stream all walk it, so a new state tensor is added in that one place.  WHICH streams move and when is the
// call's ChainPlan (chain_plan.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace se {

constexpr int kStateRowsMax = 16;  // SE_MAX_LEVELS encoder levels + 3 preconv blocks + 4 GRU layers, rounded up

struct StateRow {
    const uint32_t *src;  // row b at src + b * words; nullptr: write zeros
    uint32_t *dst;        // row b at dst + b * words
    long words;           // 4-byte words per stream row
};

struct StateRowTable {  // passed by value: the kernel-argument segment is the device table
    StateRow r[kStateRowsMax];
};

// streams: device list of stream indices (each < the allocation batch of every tensor in the table)
__global__ __launch_bounds__(256) void k_state_rows(StateRowTable t, const int *streams) {
    const StateRow r = t.r[blockIdx.z];
    const long b = streams[blockIdx.y];
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x, step = (long)gridDim.x * blockDim.x;
    if ((r.words & 3) == 0) {  // rows start on 16-byte boundaries (hipMalloc bases, row size a multiple of 16 bytes)
        const uint4 *s = r.src ? reinterpret_cast<const uint4 *>(r.src + b * r.words) : nullptr;
        uint4 *d = reinterpret_cast<uint4 *>(r.dst + b * r.words);
        const long n = r.words >> 2;
        for (long i = first; i < n; i += step) d[i] = s ? s[i] : make_uint4(0u, 0u, 0u, 0u);
    } else {
        const uint32_t *s = r.src ? r.src + b * r.words : nullptr;
        uint32_t *d = r.dst + b * r.words;
        for (long i = first; i < r.words; i += step) d[i] = s ? s[i] : 0u;
    }
}

// nrows table entries x nstreams streams; max_words = the longest row of the table
inline void launch_k_state_rows(hipStream_t st, const StateRowTable &t, int nrows, const int *streams, int nstreams, long max_words) {
    if (nrows <= 0 || nstreams <= 0) return;
    const long units = (max_words + 3) / 4;
    const unsigned gx = (unsigned)std::min<long>(std::max<long>((units + 255) / 256, 1), 32);  // <= 32 workgroups per row, the rest by stride
    hipLaunchKernelGGL(k_state_rows, dim3(gx, (unsigned)nstreams, (unsigned)nrows), dim3(256), 0, st, t, streams);
}

// The rows of one launch: add() every tensor, then launch() in one direction for a device list of streams.
struct StateRowList {
    struct Row { float *live, *carry; long words; } row[kStateRowsMax];
    int n = 0;
    void add(float *live, float *carry, long words) { row[n++] = Row{live, carry, words}; }
    // dir 0: live -> carry (save), 1: carry -> live (restore), 2: zeros -> live
    void launch(hipStream_t st, int dir, const int *streams, int nstreams) const {
        StateRowTable t{};
        long wmax = 0;
        for (int i = 0; i < n; i++) {
            t.r[i].src = reinterpret_cast<const uint32_t *>(dir == 0 ? row[i].live : dir == 1 ? row[i].carry : nullptr);
            t.r[i].dst = reinterpret_cast<uint32_t *>(dir == 0 ? row[i].carry : row[i].live);
            t.r[i].words = row[i].words;
            wmax = std::max(wmax, row[i].words);
        }
        launch_k_state_rows(st, t, n, streams, nstreams, wmax);
    }
};

}  // namespace se
