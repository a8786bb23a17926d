// pipe_lanes.h — the lanes of a host-scheduled phase (K3's factorisation, K4's column loop) and the recorder of its launch plan.
#pragma once
#include <string.h>
#include "pipe_streams.h"

namespace llmc {

#define LLMC_TRY(expr) do { if (int _rc = (expr)) return _rc; } while (0)

enum Lane {
    CHAIN = 0,   // the latency-bound chain and what it needs next. The caller's stream
    BULK = 1,    // throughput-bound work the chain does not wait for: a helper stream (pipe_streams.h), or without helper streams the chain stream
    CALLER = 2,  // the caller's stream where the chain is not (NULL-stream caller with CU-masked helpers: pipe_chain_stream)
    RIDE = 3     // no stream (K4): on the in-block launches of the NEXT group (k_gptq_block_riders), one slice per launch
};

// The launches of one call in issue order, for tests: with a recorder a phase launches nothing and touches no device. A row is
// `w` int32 that the phase's sink composes (include/llmc_hip_test.h has the layouts), with `lanes` one more: the lane. Then there
// are event rows too: `blank` with PLAN_RECORD or PLAN_WAIT as the kind and the event's id in the second field.
enum { PLAN_RECORD = 5, PLAN_WAIT = 6 };
struct PlanRec {
    int32_t* out; int cap, n, w; bool lanes; const int32_t* blank;
    void row(const int32_t* v, int lane) {
        if (n < cap) {
            int32_t* r = out + (size_t)n * (w + lanes);
            memcpy(r, v, (size_t)w * sizeof(int32_t));
            if (lanes) r[w] = lane;
        }
        ++n;
    }
    void event(int kind, int id, int lane) {
        int32_t v[32];      // w <= 32
        memcpy(v, blank, (size_t)w * sizeof(int32_t));
        v[0] = kind, v[1] = id;
        row(v, lane);
    }
};

// The chain and bulk streams of a call, and the events between them. Three forms: real helper streams (PipeStreams); one stream,
// where both lanes are the caller's stream and record / wait do nothing; the laned plan, where an event is an integer id that
// is written down. Either way a phase states its dependencies once.
struct Ev { hipEvent_t h; int id; };      // {}: nothing to wait for
struct Lanes {
    hipStream_t s[3];
    PipeStreams* ps = nullptr; PlanRec* plan = nullptr; int ids = 0;
    Lanes(hipStream_t st, PlanRec* rec) : s{st, st, st} {
        if (rec && rec->lanes) {
            plan = rec;
            s[BULK] = (hipStream_t)(uintptr_t)1;     // only ever compared (lane_of): a recorder launches nothing
        } else if (!rec && helper_streams_enabled() && (ps = pipe_streams_for(st))) {
            s[CHAIN] = pipe_chain_stream(ps, st);
            s[BULK] = ps->bulk;
        }
    }
    bool piped() const { return s[BULK] != s[CHAIN]; }
    int lane_of(hipStream_t st) const { return st == s[CHAIN] ? CHAIN : BULK; }
    int record(Lane l, Ev* e) {
        if (ps) return ps->record(s[l], &e->h);
        if (plan) plan->event(PLAN_RECORD, e->id = ++ids, lane_of(s[l]));
        return LLMC_OK;
    }
    int wait(Lane l, const Ev& e) {
        if (ps) return pipe_wait(s[l], e.h);
        if (plan && e.id) plan->event(PLAN_WAIT, e.id, lane_of(s[l]));
        return LLMC_OK;
    }
    int order(Lane first, Lane then) {      // what `then` issues from here on comes after everything `first` has issued
        Ev e{};
        LLMC_TRY(record(first, &e));
        return wait(then, e);
    }
    // Both lanes start behind the caller's earlier work, and everything is fenced back into the caller's stream before the entry
    // point returns: the C ABI contract (complete, in stream order, on the stream passed in)
    int fork() {
        Ev e{};
        LLMC_TRY(record(CALLER, &e));
        if (s[CHAIN] != s[CALLER]) LLMC_TRY(wait(CHAIN, e));
        return wait(BULK, e);
    }
    int join() {
        LLMC_TRY(order(BULK, CHAIN));
        return s[CHAIN] == s[CALLER] ? LLMC_OK : order(CHAIN, CALLER);
    }
};

}  // namespace llmc
