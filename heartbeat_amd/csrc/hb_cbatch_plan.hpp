// hb_cbatch_plan.hpp -- the planner of the batched calls: which items go
// through the batch path, how they fall into groups and where each item's
// evaluations sit in its group (hb_batch_groups: all six hb_*_many calls), and
// a group's queue of wave-jobs (hb_cbatch_jobs: hb_cxx_encode_many,
// hb_cxx_prove_many, hb_cxx_verify_rhs_many; hb_cbatch_plan is both).  Pure
// host functions: no HIP, no context, no allocation beyond their result, so
// that a stand-alone program can walk it (tests/cbatch/plan_main.cpp, built
// with AddressSanitizer and UBSan).
//
// A wave-job is up to HB_CB_JOB evaluations [first, first + count) of one item
// under one key (one kind): what one wave of hb_cbatch_prf_kernel takes from
// the queue with one atomic, so that the key schedule it reads is wave-uniform.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

// Evaluations per wave-job: a multiple of the 64 lanes of a wave.  At 64 every
// lane runs one evaluation to its end (the plain per-lane loop); above, lanes
// whose evaluation is accepted take the wave-job's next one (DESIGN.md 5.3d
// has the A/B).
#ifndef HB_CB_JOB
#define HB_CB_JOB 64
#endif
static_assert(HB_CB_JOB >= 64 && HB_CB_JOB % 64 == 0, "HB_CB_JOB is a multiple of the wave size");

// kinds of a wave-job (also its queue slot: tries)
#define HB_CB_F 0u                // F(k) = cxx prf(f_key, p)(k), k < blocks
#define HB_CB_ALPHA 1u            // alpha_j = cxx prf(alpha_key, p)(j), j < S
// the batched cxx prove and verify (hb_cpv.hpp); an encode item has none
#define HB_CB_V 2u                // v_i = cxx prf(chal_key, v_max)(i), i < chunks
#define HB_CB_IDX 3u              // idx_i = cxx prf(chal_key, ntags)(i): prove, sampled
#define HB_CB_IDXF 4u             // F(idx_i), the index drawn in the same lane (check_all: F(i)): verify
#define HB_CB_KINDS 5u

// The device reads this table entry as four dwords (hb_load_uniform).
struct HbCbJob {
    uint32_t item;                // position of the item inside its group
    uint32_t kind, first, count;
};

// What the planner has to know of one item.
struct HbCbItemReq {
    uint64_t n[HB_CB_KINDS];      // evaluations per kind (each < 2^32)
    uint32_t aes[HB_CB_KINDS];    // AES blocks per try of that kind: ByteCount(limit) / 16
    uint64_t units;               // what the group cap and the fall-through bound count (encode: blocks)
    uint64_t bytes;               // device scratch the item needs inside a group
};

struct HbCbGroup {
    uint64_t item0, nitems;       // the group's items: order[item0, item0 + nitems)
    uint64_t job0, njobs;         // the group's queue: jobs[job0, job0 + njobs), longest first
    uint64_t units, bytes;
};

struct HbCbPlan {
    std::vector<uint64_t> order;      // batched items, group by group, in the caller's order
    std::vector<uint64_t> ubase;      // per entry of `order`: units of the group's items before it
    std::vector<uint64_t> through;    // items the batch path does not take, in the caller's order
    std::vector<HbCbGroup> groups;
    std::vector<HbCbJob> jobs;
};

// Which items the batch path takes and how they fall into groups: every batched
// call's first question (the wave-job queue below is the cxx calls' second).
// unit_bound: items with more units fall through.  cap_units / cap_bytes: a
// group ends before the item that would take it over either (an item alone
// may exceed them: every batched item gets a group).  The callers pass
// unit_bound <= cap_units.  The result has no wave-jobs yet (jobs empty, every
// group's job0 = njobs = 0).
inline HbCbPlan hb_batch_groups(const HbCbItemReq *items, uint64_t nitems, uint64_t unit_bound, uint64_t cap_units,
                                uint64_t cap_bytes) {
    HbCbPlan P;
    uint64_t i = 0;
    while (i < nitems) {
        HbCbGroup G = {P.order.size(), 0, 0, 0, 0, 0};
        for (; i < nitems; ++i) {
            const HbCbItemReq &R = items[i];
            if (R.units > unit_bound) {
                P.through.push_back(i);
                continue;
            }
            if (G.nitems && (R.units > cap_units || G.units > cap_units - R.units || R.bytes > cap_bytes ||
                             G.bytes > cap_bytes - R.bytes))
                break;
            P.order.push_back(i);
            P.ubase.push_back(G.units);
            ++G.nitems;
            G.units += R.units;
            G.bytes += R.bytes;
        }
        if (!G.nitems) break;
        P.groups.push_back(G);
    }
    return P;
}

// The cxx calls' wave-job queues: HB_CB_JOB evaluations of one item and kind
// each, per group longest first.  An item without any evaluation still belongs
// to its group (its outputs may need writing) but gets no wave-job.
inline void hb_cbatch_jobs(const HbCbItemReq *items, HbCbPlan &P) {
    for (HbCbGroup &G : P.groups) {
        G.job0 = P.jobs.size();
        const uint64_t *ord = P.order.data() + G.item0;
        for (uint64_t f = 0; f < G.nitems; ++f) {
            const HbCbItemReq &R = items[ord[f]];
            for (uint32_t k = 0; k < HB_CB_KINDS; ++k)
                for (uint64_t a = 0; a < R.n[k]; a += HB_CB_JOB) {
                    const uint64_t left = R.n[k] - a;
                    P.jobs.push_back(HbCbJob{(uint32_t)f, k, (uint32_t)a, (uint32_t)(left < HB_CB_JOB ? left : HB_CB_JOB)});
                }
        }
        G.njobs = P.jobs.size() - G.job0;
        // longest wave-job first: a try's AES blocks, then the fuller wave-job
        // (its wave lasts as long as the longest of `count` rejection chains)
        std::stable_sort(P.jobs.begin() + (ptrdiff_t)G.job0, P.jobs.end(), [&](const HbCbJob &a, const HbCbJob &b) {
            const uint32_t la = items[ord[a.item]].aes[a.kind], lb = items[ord[b.item]].aes[b.kind];
            return la != lb ? la > lb : a.count > b.count;
        });
    }
}

inline HbCbPlan hb_cbatch_plan(const HbCbItemReq *items, uint64_t nitems, uint64_t unit_bound, uint64_t cap_units,
                               uint64_t cap_bytes) {
    HbCbPlan P = hb_batch_groups(items, nitems, unit_bound, cap_units, cap_bytes);
    hb_cbatch_jobs(items, P);
    return P;
}
