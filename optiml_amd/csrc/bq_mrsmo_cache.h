// The row cache of the batched row-based SMO (bq_mrsmo.hip): ONE resolution of all the rows a phase of a step asks for, one
// definition for the device (the last workgroup of a launch) and for the host check (tests/c/mrsmo_cache_check.cpp, run by
// tests/test_mrsmo_cache_host.py).  No HIP types.
//
// A call takes the pins (slots of rows the step in hand still reads: the i rows while the j rows are resolved) and m requests (a
// row, or -1: none), and gives every request its slot:
//   0. the pins are stamped again (no hit is counted: nobody asked for them);
//   1. in request order, every request whose row is in the cache is a hit and its slot is stamped;
//   2. in request order, every other request is a miss and takes a victim — slots never used first, in order, then the victim of
//      bq_rsmo_step.h (smallest stamp, lower slot among equals) among the slots NOT stamped in this call — unless an earlier request
//      of this call brought the same row in: then it shares that slot and is a hit.
// Every slot a request or a pin of this call names is stamped in this call, so none of them can be evicted by it: R >= pins +
// distinct requested rows is all a call needs.  The clock advances by one per stamp.  The distinct missing rows and their slots
// are appended to the miss list, which the row-block kernel reads.
//
// PAR is how the victim scan is shared out: the device hands the slots to the threads of the workgroup (every thread calls with
// the same arguments; thread 0 writes, barriers in between), the host is one thread.
#pragma once
#include "bq_rsmo_step.h"

struct bq_mrsmo_cache {
    long long R, clock, hits, misses, filled;
    int *slot_of;       // per row: its slot or -1
    int *row_of;        // per slot: its row or -1
    long long *stamp;   // per slot: the clock of its last use, 0 = never
};

struct bq_mrsmo_serial {   // the host's PAR
    int tid() const { return 0; }
    int size() const { return 1; }
    void sync() const {}
    void pick(long long *, long long *) const {}   // the arg-min over the threads' candidates, given to every thread
};

template <typename PAR>
BQ_RSMO_FN void bq_mrsmo_resolve(bq_mrsmo_cache *c, int np, const int *pin, int m, const int *req_row, int *req_slot, int *miss_row,
                                 int *miss_slot, int *n_miss, PAR &par) {
    const long long clock0 = c->clock, R = c->R;
    par.sync();   // every thread holds clock0
    if (par.tid() == 0) {
        long long clock = clock0, hits = 0;
        for (int q = 0; q < np; ++q)
            if (pin[q] >= 0) c->stamp[pin[q]] = ++clock;
        for (int q = 0; q < m; ++q) {
            const int r = req_row[q], have = r >= 0 ? c->slot_of[r] : -1;
            req_slot[q] = have;
            if (have >= 0) {
                c->stamp[have] = ++clock;
                hits += 1;
            }
        }
        c->clock = clock;
        c->hits += hits;
        *n_miss = 0;
    }
    par.sync();
    for (int q = 0; q < m; ++q) {
        const int r = req_row[q];
        if (r < 0 || req_slot[q] >= 0) continue;   // uniform: written before the last barrier
        const int have = c->slot_of[r];            // >= 0: an earlier request of this call brought the row in
        const long long filled = c->filled;
        long long victim = -1, best = 0;
        if (have < 0) {
            if (filled < R) {
                victim = filled;
            } else {
                for (long long s = par.tid(); s < R; s += par.size()) {
                    const long long st = c->stamp[s];
                    if (st <= clock0 && bq_rsmo_victim_before(st, s, best, victim)) {
                        best = st;
                        victim = s;
                    }
                }
                par.pick(&best, &victim);
            }
        }
        par.sync();   // every thread has read the tables
        if (par.tid() == 0) {
            const long long now = ++c->clock;
            if (have >= 0) {
                c->stamp[have] = now;
                c->hits += 1;
                req_slot[q] = have;
            } else if (victim >= 0) {
                const int old = c->row_of[victim];
                if (old >= 0) c->slot_of[old] = -1;
                c->row_of[victim] = r;
                c->slot_of[r] = (int)victim;
                c->stamp[victim] = now;
                if (filled < R) c->filled = filled + 1;
                c->misses += 1;
                req_slot[q] = (int)victim;
                miss_row[*n_miss] = r;
                miss_slot[*n_miss] = (int)victim;
                *n_miss += 1;
            }
        }
        par.sync();
    }
}
