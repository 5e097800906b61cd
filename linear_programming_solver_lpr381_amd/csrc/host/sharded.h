// host/sharded.h -- the rank protocol of a sharded search, once (level search and warm search of bnb.cpp, rounds of knapsack.cpp).
//
// A sharded search expands its tree REPLICATED on every rank until there is enough to share (the warm-up), hands entry i of
// what it then holds to rank i % world, and from there on every rank works on its own part and meets the others in ONE
// all-reduce(MAX) per level / round.  Everything the ranks tell each other goes through that one collective (RCCL in production):
// a value only rank r knows travels in slot r of a vector the other ranks fill with -inf.
//
// The warm-up relies on every rank computing the SAME state (same LPs, same arithmetic, same decisions).  If that ever fails --
// round 2's record scale7: a kernel whose result depended on workgroup scheduling under GPU sharing gave the ranks different root
// LPs; they left the replicated phase on different levels and then sat in collectives that no longer matched until the job was
// killed -- the ranks must find out instead of waiting for good: a fingerprint of the state as it stands when the replicated phase
// ends (hand-out, or the search running dry / out of budget before it) travels as {+h, -h} in the FIRST exchange of every rank;
// max(+h) == -max(-h) iff all ranks agree.  Every rank of a sharded search issues that first exchange, also one whose search ended
// while replicated.  A rank whose own work throws does not leave either (its peers would wait in the exchange for good): it keeps
// taking part with `failed` up, all ranks stop together, and the error is thrown after the loop.
#pragma once
#include "model.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

namespace lpx { namespace host {

// Hash of the state a rank leaves the replicated phase with; each search feeds its own frontier / heap.  52 bits: exact in a double.
struct Fingerprint {
    uint64_t h;
    explicit Fingerprint(bool handed_out) : h(1469598103934665603ull ^ (handed_out ? 0x9e3779b97f4a7c15ull : 0ull)) {}
    void mix(uint64_t v) { h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2); }
    void mix_bits(double d) { int64_t b; std::memcpy(&b, &d, sizeof(b)); mix((uint64_t)b); }
    double value() const { return (double)(h & ((1ull << 52) - 1)); }
};

struct Sharded {
    const EngineOptions& opt;
    const int world, rank;
    const bool sharded;               // the exchange exists: more than one rank (or a world of one told to shard) and a collective
    bool replicated;                  // still in the warm-up every rank computes alike
    const char* const identical;      // what the warm-up needs bit-identical across ranks, for the divergence text
    int64_t allreduces = 0;           // SimplexResult::Aux
    // fingerprint of the end of the replicated phase, sent once.  Set by agree(): a world of one that never replicates (before
    // its first level / round), the hand-out, and a search ending inside the replicated phase.
    double agree_h = -1.0; bool agree_sent;
    bool failed = false; std::string fail_msg; int fail_code = 0;

    Sharded(const EngineOptions& o, const char* what_identical)
        : opt(o), world(std::max(1, o.world)), rank(o.rank), sharded((world > 1 || o.shard_one) && (bool)o.allreduce_max),
          replicated(world > 1), identical(what_identical), agree_sent(!sharded) {}

    bool mine(size_t i) const { return (int)(i % (size_t)world) == rank; }        // the hand-out
    bool exchanging() const { return sharded && !replicated; }
    void max(double* v, int n) { opt.allreduce_max(v, n); ++allreduces; }
    void agree(double h) { agree_h = h; replicated = false; }
    // this rank's own work threw: from the warm-up too, the peers meet this rank in their first exchange after the hand-out
    void fail(const LpxException& e) { failed = true; fail_msg = e.what(); fail_code = e.code; replicated = false; }
    void rethrow() const { if (failed) throw LpxException(fail_code ? fail_code : LPX_EDEVICE, fail_msg); }

    enum Verdict { GO_ON, STOP, PEER_FAILED, DIVERGED };
    struct Round { Verdict verdict; bool better; double best; };   // better: a peer holds a larger incumbent bound, `best`

    // The per-level / per-round all-reduce over `n` doubles.  Slots 0..2 are {incumbent, have work, failed} and the last two carry
    // {+h, -h} in a rank's first exchange (-inf afterwards); the caller fills what lies between (the cold level search: deepest
    // pooled node and every rank's pool size) and leaves the rest at -inf.
    // One rule for the verdict: a raised `failed` always wins; divergence is reported only when nobody failed (a failed rank sends
    // no fingerprint, which alone would look like one); only then does "nobody has work" end the search.  Every verdict but GO_ON
    // ends the loop on all ranks in the same exchange; PEER_FAILED and DIVERGED leave the error in the failure triple.
    Round exchange(double* vals, int n, double incumbent, bool have_work)
    {
        vals[0] = incumbent; vals[1] = have_work ? 1.0 : 0.0; vals[2] = failed ? 1.0 : 0.0;
        const bool first = !agree_sent;
        if (first && !failed) { vals[n - 2] = agree_h; vals[n - 1] = -agree_h; }
        agree_sent = true;
        max(vals, n);
        Round r{GO_ON, vals[0] > incumbent, vals[0]};
        if (vals[2] > 0.0) {
            if (!failed) { failed = true; fail_code = LPX_EDEVICE; fail_msg = "sharded search: a peer rank failed"; }
            r.verdict = PEER_FAILED;
        } else if (first && vals[n - 2] != -vals[n - 1]) {
            failed = true; fail_code = LPX_EDEVICE;
            fail_msg = std::string("sharded search: the replicated warm-up ended differently on different ranks (") + identical +
                       " must be bit-identical across ranks)";
            r.verdict = DIVERGED;
        } else if (vals[1] == 0.0) r.verdict = STOP;
        return r;
    }
};

}}  // namespace lpx::host
