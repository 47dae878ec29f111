// pool.hpp -- the work vectors the library keeps between solves (Pool, held as Ctx::pool) and everything the placement of the
// product's output remembers (PlaceState, held as Ctx::place).  Host only; the code is in placement.hip.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace lcgh {

// Scratch vectors of past solves, kept for the next one (hipMalloc + hipFree cost ~0.2 ms per solve, as much as ten iterations of a
// small system; lcg_hip_trim() gives them back).  The ORDER of the entries is part of the behaviour: it decides best-fit ties, the
// order of placement's candidates and with both which role receives which vector -- entries are appended and erased, never sorted.
struct Pool {
    struct Vec { double *p; size_t bytes; bool busy; void *arena; };   // arena: the allocation this vector is a slot of (placement.hip: keep_as_arena), or null
    std::vector<Vec> v;
    bool arena_busy(const void *a) const;      // one of the arena's slots is in use
    // a vector of at least `bytes`, marked busy: the smallest idle one that fits (the first of equals); else ONE idle vector that is
    // no slot of an arena is given back -- its timings forgotten, nothing counted in PlaceState::gave_back -- and a new one allocated
    int take(size_t bytes, double *&out);
    void set_busy(const double *p, bool busy) { for (auto &s : v) if (s.p == p) s.busy = busy; }
    // idle vectors of at least `bytes` in pool order, the slots of arenas first, `limit` at most
    std::vector<double *> idle(size_t bytes, size_t limit) const;
    // `count` idle slots of `slot` bytes each, cut from the allocation at `base`, which the pool owns from here on
    void add_arena(void *base, size_t slot, size_t count);
    // Two arenas at most: while two or more exist, the oldest one none of whose slots is in use goes -- one per call; true when one
    // went.  Its slots leave the pool (their timings forgotten) and are appended to `gone`, the allocation is freed.
    bool evict_idle_arena(std::vector<double *> &gone);
    // everything idle goes, the slots of an arena together once none of them is in use; returns the bytes of the entries removed
    size_t trim();
    void totals(int *vectors, int64_t *bytes, int *arena_slots) const;      // (lcg_hip_pool_info; null: not asked)
};

// Where the product's output lies (placement.hip): the memo, the walk's bounds, the mode, what the latest solve and the
// latest walk did, and how much the library has given back to the device.
struct PlaceState {
    // what y = A.x took into a given vector against a given matrix (val = the matrix's value array; y == nullptr: "this matrix has
    // had its walk, do not look again")
    struct Memo { const void *val; const double *y; float us; };
    std::vector<Memo> memo;
    float *find(const void *val, const double *y) { for (auto &m : memo) if (m.val == val && m.y == y) return &m.us; return nullptr; }
    void forget_all() { memo.clear(); }
    // one vector left the pool: its timings go, the per-matrix "has had its walk" markers (y == nullptr) stay
    void forget_vector(const double *y) { for (size_t i = 0; y && i < memo.size();) if (memo[i].y == y) memo.erase(memo.begin() + (long)i); else i++; }
    // Bounds of the placement's walk (placement.hip: walk).  Production values; lcg_hip_placement_tune_for_test lowers them so
    // that the walk, the arenas and their eviction run under -m gpu at a few million rows.
    struct Tune {
        size_t stream_min = (size_t)768 << 20;     // a product that streams less shows one kind of place only: nothing is timed
        size_t chunk = (size_t)1 << 30;            // the walk's step
        int max_chunks = 128;
        double wall_ms = 60.0;                     // looked at after EVERY allocation of the walk
        size_t hold_max = (size_t)64 << 30;        // what a walk may hold at once: this many bytes ...
        double hold_frac = 0.25;                   // ... and this fraction of the memory that was free when it started
        size_t keep_free = (size_t)8 << 30;        // never into the last bytes of free memory
        size_t shared_min = (size_t)4 << 30;       // others held more than this when the library was initialised: the device is shared, no walk
        bool predict = true;                       // another chunk only while time used + the dearest allocation so far <= wall_ms
        size_t released_max = (size_t)1 << 30;     // the library has given back more than this in the process's life: no walk (below)
        int force_find_at = -1;                    // test hook: the k-th TIMED chunk is taken as the faster place whatever the clock says
    } tune;
    int mode = -1;                     // lcg_hip_set_placement: -1 auto (large products on one GPU), 0 never, 1 whenever the callback is the built-in one
    struct Solve {                     // the latest solve (lcg_hip_last_placement)
        int timed = 0, moved = 0;      // candidates timed (0: answered from the memo, or not tried); roles moved to another vector
        double us_first = 0.0, us_chosen = 0.0;    // the first output: as allocated / as placed
    } last;
    struct Walk {                      // walks made so far, and the latest (lcg_hip_last_placement_walk)
        int made = 0, chunks = 0, found = 0;       // chunks allocated; 1 = a faster place was kept
        double ms = 0.0; size_t held = 0; const char *end = "";    // wall time; most bytes held at once; why it ended
    } walk;
    // What the library has handed back to the device in this process's life (matrices destroyed, pool vectors and arenas trimmed, the
    // chunks of an earlier walk).  A 1 GiB hipMalloc costs 0.1-0.5 ms out of memory the process has never held and 30 ms .. 0.5 s ONE
    // CALL once the allocator recycles what was released (bench.py's variants, LCG_HIP_DEBUG=1: walks of 74 / 381 / 528 ms against a
    // bound of 60 that can only be looked at between calls) -- so the walk is made while the allocator is fresh: in practice once per
    // process, for its first large system.
    size_t released_bytes = 0;
    // The one place the sum grows.  The walk's "fresh allocator" rule needs the order of magnitude, and the six sites that give
    // memory back do not count alike (tests/test_gpu_placement.py: test_no_walk_once_the_library_has_given_memory_back depends on
    // these sums as they are):
    //   1. lcg_hip_trim (placement.hip)            the bytes of every pool entry removed, each slot of an arena with its own
    //   2. the walk's chunks (placement.hip: walk) Tune::chunk for every chunk given back
    //   3. a kept chunk whose walk failed (walk)   Tune::chunk
    //   4. an evicted arena (keep_as_arena)        Tune::chunk as it is NOW, whatever the arena's allocation measured
    //   5. lcg_hip_csr_destroy (csr.hip)           nnz x 12 (complex: x 20) of the main part; the plans beside it are not counted
    //   6. the eviction in Pool::take              nothing
    void gave_back(size_t bytes) { released_bytes += bytes; }
    bool ranks_share_device = false;               // two ranks of the communicator / of the mailboxes sit on this device (comm.hip: found at connect time)
    size_t mem_total = 0, mem_free_at_init = 0;    // hipMemGetInfo at ensure_init: total - free = what others (and the host program) held
};

} // namespace lcgh
