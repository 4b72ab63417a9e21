// chain_plan.h - the host-side plan of one realtime_process call over a batch whose streams have their own lengths (and flags).
//
// Both inference engines (se_engine.hip, fsn_engine.inc.h) cut a stream into half-overlapping segments of K samples.  A stream that
// continues its carried state starts K/2 before its first sample; one that is reset gets K/2 zeros in front (the lead), which the
// overlap average strips again.  chunk_geometry() is the ONE place that arithmetic lives (utility.py:327-329, 360-368; CRN.py:568-570);
// engine.chain_geometry restates it in Python and tests/test_chain_plan_cpu.py holds the two together through se_chunk_geometry.
//
// A ChainPlan is everything a call needs beyond the uniform case:
//   nseg[b]      segments stream b takes part in (the count it has alone); N = the most any stream has
//   le[k]        streams with at most k segments, k = 0 .. N
//   sorted       device: the streams by ascending segment count (stable), so the streams whose LAST segment is n are positions
//                [le[n], le[n + 1]) of it: ending(n).  Their state rows are saved there and restored at call exit (ended_early())
//   zeroed       device: the nzero streams with flag 0, whose rows are zeroed at entry when other streams continue
//   len / off0 / skip   device int64 [B]: own length, offset of the first segment in the stream, samples stripped by the overlap average
//   compact      the streams still running in segment n are a PREFIX of the batch (counts non-increasing): launches cover bact(n) streams
//   saving       some stream ends before the longest one: save / restore is live
// plan_chains() validates, sorts and fills `staging` = len | off0 | skip | (int) sorted | zeroed; the engine uploads it with one copy
// into 8 * B floats of its own and calls carve() (engine_host.h: upload_plan).  A ragged call (se_realtime_process_ragged: a common flag,
// lengths only) is a chains call whose flags are all equal.  Plain host C++: no HIP types, no engine types.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/se_engine.h"

namespace se {

static_assert(sizeof(long) == sizeof(int64_t), "per-stream geometry is passed to the kernels as long");

struct ChunkGeometry { long nseg, off0, skip; };

inline ChunkGeometry chunk_geometry(long K, long length, bool continues) {
    const long P = K / 2, lead = continues ? 0 : P;  // CRN.py:568-570
    const long Lp = length + lead;
    const long gap = K - (P + Lp % K) % K;           // utility.py:327-329
    // segment n covers padded[n*P, n*P+K) with padded = [0]*P | [0]*lead | x | zeros; the strip is the lead (CRN.py:587-588)
    return {2 * (Lp + gap + P) / K, -P - lead, lead};  // utility.py:360-368
}

struct StreamRange { const int *streams; int count; };  // a run of a device stream list

struct ChainPlan {
    int B = 0, N = 0, nzero = 0;
    std::vector<int> nseg, le;
    bool compact = false, saving = false;
    const long *len = nullptr, *off0 = nullptr, *skip = nullptr;
    const int *sorted = nullptr, *zeroed = nullptr;
    std::vector<int64_t> staging;

    bool continues() const { return nzero < B; }  // some stream carries state into the call
    int bact(long n) const { return compact ? std::max(B - le[n], 1) : B; }
    StreamRange ending(long n) const {  // (the call's last segment saves nothing: those streams' state is already where it belongs)
        return saving && n + 1 < N ? StreamRange{sorted + le[n], le[n + 1] - le[n]} : StreamRange{nullptr, 0};
    }
    StreamRange ended_early() const { return {sorted, saving ? le[N - 1] : 0}; }
    StreamRange reset_streams() const { return {zeroed, nzero}; }
    size_t staging_floats() const { return (size_t)8 * B; }
    void carve(const void *dev) {  // dev: the uploaded staging vector
        len = static_cast<const long *>(dev); off0 = len + B; skip = len + 2 * (size_t)B;
        sorted = reinterpret_cast<const int *>(len + 3 * (size_t)B); zeroed = sorted + B;
    }
};

enum { kPlanFilled = 0, kPlanUniform = 1 };

// One flag and one length per stream; `carried` = the streams whose state the engine holds (<= 0: none).  Returns kPlanFilled with p
// complete but for carve(), kPlanUniform with *uniform_flag when every stream has max_length and the same flag (the plain call serves
// it), or an SE_ERR_* code with its text in err.
inline int plan_chains(ChainPlan &p, long K, int batch, int64_t max_length, const int64_t *lengths, const uint8_t *flags, int carried,
                       int *uniform_flag, std::string &err) {
    for (int b = 0; b < batch; b++)
        if (lengths[b] <= 0 || lengths[b] > max_length) {
            char buf[128];
            snprintf(buf, sizeof buf, "length of stream %d (%lld) outside (0, %lld]", b, (long long)lengths[b], (long long)max_length);
            err = buf;
            return SE_ERR_ARG;
        }
    bool any = false, all = true, full = true;
    for (int b = 0; b < batch; b++) {
        any = any || flags[b];
        all = all && flags[b];
        full = full && lengths[b] == max_length;
    }
    if (any && carried <= 0) { err = "a stream continues (flag set) but the engine carries no state"; return SE_ERR_STATE; }
    if (any && carried != batch) {
        err = "a stream continues (flag set) in a batch of " + std::to_string(batch) + " but the carried state holds " + std::to_string(carried) + " streams";
        return SE_ERR_STATE;
    }
    if (full && (all || !any)) { *uniform_flag = all ? 1 : 0; return kPlanUniform; }
    // every stream keeps the geometry it has alone
    const size_t B = (size_t)batch;
    p = ChainPlan{};
    p.B = batch;
    p.nseg.resize(B);
    p.staging.assign(4 * B, 0);
    std::vector<int> idx(2 * B, 0);
    for (int b = 0; b < batch; b++) {
        const ChunkGeometry g = chunk_geometry(K, lengths[b], flags[b]);
        p.nseg[b] = (int)g.nseg;
        p.N = std::max(p.N, p.nseg[b]);
        p.staging[b] = lengths[b];
        p.staging[B + b] = g.off0;
        p.staging[2 * B + b] = g.skip;
        idx[b] = b;
        if (!flags[b]) idx[B + p.nzero++] = b;
    }
    std::stable_sort(idx.begin(), idx.begin() + B, [&](int a, int b) { return p.nseg[a] < p.nseg[b]; });
    memcpy(p.staging.data() + 3 * B, idx.data(), 2 * B * sizeof(int));
    p.le.assign((size_t)p.N + 1, 0);
    for (int b = 0; b < batch; b++) p.le[p.nseg[b]]++;
    for (int k = 1; k <= p.N; k++) p.le[k] += p.le[k - 1];
    p.saving = p.le[p.N - 1] > 0;
    // prefix compaction: the streams still running in segment n are a prefix of the batch when the SEGMENT COUNTS are non-increasing (a
    // reset stream has one lead more than a continuing one); the streams beyond the prefix are exactly those whose rows were saved
    p.compact = true;
    for (int b = 1; b < batch; b++) p.compact = p.compact && p.nseg[b] <= p.nseg[b - 1];
    return kPlanFilled;
}

}  // namespace se
