// placement.hip -- the work-vector pool (pool.hpp: Pool), the placement of the product's output over it (place_roles, called by
// driver.hpp: Solve::place) and the exported entries of both.  Host code only: the products it times are csr.hip's.
#include "driver.hpp"

namespace lcgh {

// ---- the pool ----------------------------------------------------------------------------------------------------------------
int Pool::take(size_t bytes, double *&out)
{
    int best = -1;
    for (size_t i = 0; i < v.size(); i++)
        if (!v[i].busy && v[i].bytes >= bytes && (best < 0 || v[i].bytes < v[best].bytes)) best = (int)i;
    if (best < 0) {
        // nothing fits: give one idle smaller vector back and allocate
        for (size_t i = 0; i < v.size(); i++)
            if (!v[i].busy && !v[i].arena) { ctx().place.forget_vector(v[i].p); (void)hipFree(v[i].p); v.erase(v.begin() + (long)i); break; }     // (gave_back: nothing, site 6)
        double *p = nullptr;
        HIPCHK(hipMalloc(&p, bytes));
        v.push_back({p, bytes, false, nullptr});
        best = (int)v.size() - 1;
    }
    v[best].busy = true;
    out = v[best].p;
    return 0;
}

std::vector<double *> Pool::idle(size_t bytes, size_t limit) const
{
    std::vector<double *> out;
    for (int pass = 0; pass < 2; pass++)
        for (auto &s : v)
            if (!s.busy && s.bytes >= bytes && (s.arena != nullptr) == (pass == 0) && out.size() < limit) out.push_back(s.p);
    return out;
}

void Pool::add_arena(void *base, size_t slot, size_t count)
{
    for (size_t i = 0; i < count; i++) v.push_back({reinterpret_cast<double *>(static_cast<char *>(base) + i * slot), slot, false, base});
}

bool Pool::arena_busy(const void *a) const { for (auto &s : v) if (s.arena == a && s.busy) return true; return false; }

bool Pool::evict_idle_arena(std::vector<double *> &gone)
{
    int arenas = 0;
    void *victim = nullptr;
    for (auto &s : v)
        if (s.arena && s.p == s.arena) { arenas++; if (!victim && !arena_busy(s.arena)) victim = s.arena; }    // (an arena's first slot lies at its base)
    if (arenas < 2 || !victim) return false;
    for (size_t i = 0; i < v.size();)
        if (v[i].arena == victim) { ctx().place.forget_vector(v[i].p); gone.push_back(v[i].p); v.erase(v.begin() + (long)i); } else i++;
    (void)hipFree(victim);
    return true;
}

size_t Pool::trim()
{
    size_t bytes = 0;
    for (auto it = v.begin(); it != v.end();) {
        if (it->busy || (it->arena && arena_busy(it->arena))) { ++it; continue; }
        if (!it->arena || it->p == it->arena) (void)hipFree(it->p);
        bytes += it->bytes;
        it = v.erase(it);
    }
    return bytes;
}

void Pool::totals(int *vectors, int64_t *bytes, int *arena_slots) const
{
    int64_t b = 0; int a = 0;
    for (auto &s : v) { b += (int64_t)s.bytes; a += s.arena != nullptr; }
    if (vectors) *vectors = (int)v.size();
    if (bytes) *bytes = b;
    if (arena_slots) *arena_slots = a;
}

// ---- where the work vectors lie (lcg_hip.h: lcg_hip_set_placement; profiles/r04_placement.txt) -------------------
// The time of a large y = A.x depends on WHICH allocation y is: 520-530 us or 580-595 us for the headline system, constant for
// the lifetime of the pair (value array, y).  The device's memory falls into THREE groups of 96 GiB (the three ranks of its 12-high
// HBM stacks, by every sign: one group a single stretch, the other two interleaved in runs of 2-8 GiB -- scripts/placement_lab7.hip
// over 250 allocations of 1 GiB), and a vector that lies in the group of the matrix's value array is slow to write while that array
// streams (scripts/placement_lab6.hip: six read buffers x sixteen written ones fall into matching groups).  Nothing the process can
// see -- virtual address, size, allocation call -- tells the group; only the clock does.  Inside the CG loop
// (scripts/placement_roles.py, every combination of classes for g, d, A.d): A.d beside the values costs 9 % of the iteration rate
// whatever the others do, d (the product's x, and the direction pass's output) 2.6 %, g 1.3 %.  The solvers allocate their work
// vectors anyway: before the first iteration each is classed by the product's time into it, and the roles are dealt in that order
// of weight -- products' outputs first, then the vector the product reads, then the rest -- the vectors outside the value array's
// group going to the heaviest roles.  No arithmetic changes.
namespace {

constexpr float SAME = 1.03f;       // a role changes hands for 3 %
constexpr float CLASS = 1.06f;      // two KINDS of places lie 8-12 % apart (timings of one kind spread by up to 4 %): what starts a walk and ends it

// the rows this process multiplies by itself: the whole matrix, or -- sharded -- the entries with locally owned columns
const CsrPart &part(const lcg_hip_csr *A) { return A->distributed ? A->loc : A->main; }
// the effect needs a stream far larger than the 256 MB Infinity Cache: at the 8-way shard size of the 10M-row system (490 MB streamed,
// 10 MB written) eighteen candidates and a whole walk showed ONE kind of place, 69.9-71.8 us (profiles/r04_placement.txt, section 10)
bool streams(Ctx &c, const lcg_hip_csr *A) { return (size_t)part(A).nnz * 12 >= c.place.tune.stream_min; }
// the mean row length the solver's loop hands the product (a shard's local-column part has its own: comm.hip) -- the kernel
// shape that is timed here must be the one the loop runs
double mean_of(const lcg_hip_csr *A) { return A->distributed ? (A->n_rows ? (double)A->loc.nnz / A->n_rows : 0.0) : A->mean_row; }

bool wanted(Ctx &c, int n, const void *afp, const void *inst)
{
    if (c.place.mode == 0 || afp != (const void *)lcg_hip_csr_ax || inst == nullptr) return false;
    const lcg_hip_csr *A = static_cast<const lcg_hip_csr *>(inst);
    if (A->is_complex || A->c64 || n != A->n_rows || n < 4096) return false;
    return c.place.mode > 0 || streams(c, A);
}

// One solve's placement, step by step (run).  cand: the solve's own roles by weight (n_own of them), then idle vectors of the pool.
struct Placing {
    struct Cand { double **role; double *p; float us; };
    Ctx &c; PlaceState &S; const PlaceState::Tune &T;
    const lcg_hip_csr *A; const double *x; const size_t bytes; const void *val;      // the matrix, a finite n-vector, a vector's bytes, the value array
    std::vector<Cand> cand;
    size_t n_own = 0;
    float lo = 0.f, hi = 0.f;       // the fastest and the slowest candidate
    bool alike = false;             // all candidates of one kind (then nobody knows which)

    Placing(Ctx &c_, int n, void *inst, const double *x_)
        : c(c_), S(c_.place), T(c_.place.tune), A(static_cast<const lcg_hip_csr *>(inst)), x(x_), bytes(sizeof(double) * (size_t)n), val(part(A).val) {}

    int product(double *y) { return spmv_launch(part(A), false, A->variant, mean_of(A), x, y, false, c.stream, nullptr); }
    // what y = A.x takes into `y`: one product to warm up, two timed (x: the right-hand side)
    int time_output(double *y, float *us)
    {
        if (float *m = S.find(val, y)) { *us = *m; return 0; }
        hipEvent_t e0, e1;
        if (hipEventCreate(&e0) != hipSuccess) { (void)hipGetLastError(); return LCG_HIP_E_RUNTIME; }
        if (hipEventCreate(&e1) != hipSuccess) { (void)hipGetLastError(); (void)hipEventDestroy(e0); return LCG_HIP_E_RUNTIME; }
        int rc = product(y);
        if (!rc) rc = hipEventRecord(e0, c.stream) == hipSuccess ? 0 : LCG_HIP_E_RUNTIME;
        for (int i = 0; i < 2 && !rc; i++) rc = product(y);
        if (!rc && (hipEventRecord(e1, c.stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess)) rc = LCG_HIP_E_RUNTIME;
        float ms = 0.f;
        if (!rc && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = LCG_HIP_E_RUNTIME;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        if (rc) return rc;
        *us = ms * 500.f;
        S.memo.push_back({val, y, *us});
        S.last.timed++;
        return 0;
    }

    // Roles whose vector the caller supplied stay where they are; false: no product's output is the library's own, nothing to place
    bool candidates(const Workspace &ws, std::initializer_list<double **> roles, int n_out)
    {
        int k = 0, out_owned = 0;
        for (double **r : roles) { if (ws.owns(*r)) { cand.push_back({r, *r, 0.f}); if (k < n_out) out_owned++; } k++; }
        if (out_owned == 0) return false;
        n_own = cand.size();
        // idle vectors of the pool: the slots of arenas first (each was the fast place of SOME matrix), six at most -- a process that has
        // multiplied many matrices must not time its whole history against the next one
        for (double *p : c.pool.idle(bytes, 6)) cand.push_back({nullptr, p, 0.f});
        return true;
    }

    // the first output's time as allocated; *go = false: nothing a place could give shows on the clock
    int gate(bool *go)
    {
        // the plan of a matrix is built by its first product: not on the clock
        if (part(A).last_kernel[0] == 0) TRY(product(cand[0].p));
        // What a better place can give is what the written vector costs in the worse one: 60 us per 80 MB (0.75 us per MiB).  Where that is
        // less than 4 % of the product -- the two-pass binned product at 1.75 ms, bands a million columns wide -- the kinds cannot be
        // told apart by the clock and nothing is tried (39 vectors timed and 64 chunks walked for nothing, 0.3 s, before this line).
        TRY(time_output(cand[0].p, &cand[0].us));
        S.last.us_first = S.last.us_chosen = cand[0].us;
        *go = !(S.mode < 0 && 0.75 * ((double)bytes / 1048576.0) < 0.04 * cand[0].us);      // (automatic mode: a forced placement always tries)
        if (!*go && debug_on()) fprintf(stderr, "[lcg_hip] placement: not tried (a product of %.0f us writes %.0f MiB: nothing a place could give shows on the clock)\n", cand[0].us, bytes / 1048576.0);
        return 0;
    }

    int time_all()
    {
        for (auto &q : cand) TRY(time_output(q.p, &q.us));
        lo = hi = cand[0].us;
        for (auto &q : cand) { lo = std::min(lo, q.us); hi = std::max(hi, q.us); }
        alike = hi < lo * CLASS;
        return 0;
    }

    // Not enough vectors outside the value array's group (or all alike: then nobody knows which kind they are).  What is allocated
    // one after the other lies side by side, so the library walks: chunks of 1 GiB, one after the other and all held, the product
    // timed into the start of every fourth, until one is clearly faster than our slow kind (or, all alike, clearly slower: then
    // ours are the fast kind) -- within hard bounds (PlaceState::Tune: 128 chunks, 60 ms looked at after every allocation, 64 GiB and a quarter
    // of the free memory held at once, never into the last 8 GiB, not at all on a device somebody else uses).  Larger steps
    // do not get further: an allocation of 4 GiB or more costs 30 ms per GiB, and the allocator serves small requests from near-by
    // memory whatever is held elsewhere.  The fast chunk is KEPT and cut into vectors for this and later solves (one group
    // throughout: a 4 GiB allocation walked in steps of 64 MB never changes class); everything else is given back at once.  One
    // walk per matrix.
    bool walk_wanted()
    {
        size_t n_slow = 0;
        for (size_t i = 0; i < n_own; i++) if (cand[i].us > lo * CLASS) n_slow++;
        bool walk = streams(c, A) && (alike || n_slow > 0 || T.force_find_at >= 0) && S.find(val, nullptr) == nullptr && bytes <= T.chunk / 4;
        if (walk && T.shared_min != ~(size_t)0 && (S.ranks_share_device || (S.mem_total > 0 && S.mem_total - S.mem_free_at_init > T.shared_min))) {
            // somebody else lives on this device (other ranks, another framework's pool): what the walk holds, they cannot have
            if (debug_on()) fprintf(stderr, "[lcg_hip] placement walk: not made, the device is shared (%s; %.1f GiB were in use when the library was initialised)\n",
                                    S.ranks_share_device ? "another rank of this job sits on it" : "memory in use by others",
                                    (double)(S.mem_total - S.mem_free_at_init) / 1073741824.0);
            walk = false;
            S.memo.push_back({val, nullptr, 0.f});        // (decided once per matrix)
        }
        if (walk && T.released_max != ~(size_t)0 && S.released_bytes > T.released_max) {
            if (debug_on()) fprintf(stderr, "[lcg_hip] placement walk: not made, the library has given back %.1f GiB in this process (allocations out of recycled memory "
                                    "cost 30-500 ms a call; the walk is for a fresh allocator: the first large system of a process)\n", (double)S.released_bytes / 1073741824.0);
            walk = false;
            S.memo.push_back({val, nullptr, 0.f});
        }
        return walk;
    }

    // ---- the walk ----
    struct Walk {
        std::vector<double *> chunks;       // held, to be given back
        double *found = nullptr; float found_us = 0.f, ours = 0.f;      // the best chunk so far; the kind to get away from
        std::chrono::steady_clock::time_point w0 = std::chrono::steady_clock::now();
        size_t hold_cap = 0;
        int timed_chunks = 0, since_find = 0, slower_seen = 0, rc = 0;
        double alloc_sum = 0.0, alloc_max = 0.0;
        double elapsed() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count(); }
    };
    void end(const Walk &w, const char *why) { S.walk.end = w.found ? "found" : why; }

    // HARD BOUNDS, each looked at after every single allocation: T.max_chunks chunks; T.wall_ms on the clock (a chunk costs
    // 0.02-0.5 ms out of memory nobody has held since the node was provisioned, 30 ms once the driver has to clear it); what is held at once --
    // min(T.hold_max, T.hold_frac x the memory free at the start); never into the last T.keep_free bytes.  (The clock can only
    // be read BETWEEN calls: another chunk is allocated only while the time used plus the dearest allocation so far stays within
    // wall_ms, and the walk is not made at all once the allocator recycles what the library released -- PlaceState::released_bytes.)
    // false: a bound ended the walk (S.walk.end says which)
    bool next_chunk(Walk &w, int q)
    {
        const size_t CH = T.chunk;
        size_t fr = 0, tot = 0;
        if ((w.chunks.size() + 1 + (w.found ? 1 : 0)) * CH > w.hold_cap) { end(w, "hold limit"); return false; }
        if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < T.keep_free + CH) { (void)hipGetLastError(); end(w, "free-memory floor"); return false; }
        double *p = nullptr;
        const double a0 = w.elapsed();
        if (hipMalloc(&p, CH) != hipSuccess) { (void)hipGetLastError(); end(w, "allocation refused"); return false; }
        const double a1 = w.elapsed() - a0;
        w.alloc_sum += a1; w.alloc_max = std::max(w.alloc_max, a1);
        w.chunks.push_back(p);
        S.walk.chunks++;
        S.walk.held = std::max(S.walk.held, (w.chunks.size() + (w.found ? 1 : 0)) * CH);
        // (the clock is read between calls: the walk goes on only while the time used PLUS its dearest allocation so far fits the
        //  bound -- out of memory the process has held before a chunk costs 30 ms instead of 0.1-0.5)
        if (w.elapsed() + (T.predict ? w.alloc_max : 0.0) > T.wall_ms) { end(w, "wall clock"); return false; }
        // (a device whose memory has all been in use since it was booted clears every chunk it hands out, 30 ms per GiB: 128 chunks
        //  would take 4 s.  The walk pays where allocations are cheap -- freshly provisioned nodes -- and says so after ONE chunk elsewhere.)
        if (T.predict && q == 0 && a1 > 5.0) { S.walk.end = "no fresh memory"; return false; }
        return true;
    }

    // THREE kinds of places show on the clock of a product that reads a stream AND gathers x (tiled product, 10M rows: 563 / 605 /
    // 647 us -- y beside neither, beside x, beside the stream), so the first chunk that beats `ours` is not yet the answer: ours
    // 647, chunk 609 ended the round-4 walk, and the loop then ran in its slow state (687 us per product against 578 with a 563-us
    // place: profiles/r05_tiled_states.txt, one process in six).  The walk therefore keeps the BEST chunk it has seen and goes on
    // for a few timed chunks behind every find; it ends when nothing better has shown in LOOK_ON timed chunks (or at a bound).
    // The newest chunk on the clock; false: the walk has its answer (or a timing failed: w.rc)
    bool look(Walk &w)
    {
        constexpr int LOOK_ON = 3;
        double *p = w.chunks.back();
        float us = 0.f;
        w.rc = time_output(p, &us);
        if (w.rc) { S.walk.end = "timing failed"; return false; }
        const bool forced = T.force_find_at >= 0 && w.timed_chunks == T.force_find_at;
        w.timed_chunks++;
        if (forced) { w.found = p; w.found_us = 0.9f * std::min(us, lo); w.chunks.pop_back(); S.walk.end = "found"; return false; }
        if (T.force_find_at < 0) {
            // a find: clearly faster than the kind to get away from -- or, behind a find, clearly faster than that find
            const float bar = w.found ? w.found_us : w.ours;
            if (us * CLASS < bar) {
                if (w.found) w.chunks.insert(w.chunks.begin(), w.found);        // (the earlier find goes back with the others)
                w.found = p; w.found_us = us; w.chunks.pop_back(); w.since_find = 0;
            } else if (w.found) {
                if (++w.since_find >= LOOK_ON) { S.walk.end = "found"; return false; }
            } else if (alike && w.ours * CLASS < us) {
                // slower than ours: ours are not the slowest kind; after LOOK_ON such chunks and none faster, ours are taken for the fast kind
                if (++w.slower_seen >= LOOK_ON) { S.walk.end = "ours are the fast kind"; return false; }
            }
        }
        if (w.elapsed() > T.wall_ms) { end(w, "wall clock"); return false; }
        return true;
    }

    // the walk itself: *found (with its time) is the chunk to keep, or null; everything else it held is given back, S.walk is its report
    int walk(double **found, float *found_us)
    {
        const size_t CH = T.chunk;
        Walk w;
        w.ours = alike ? lo : hi;
        size_t fr0 = 0, tot = 0;
        S.walk.made++;
        S.walk.chunks = 0; S.walk.found = 0; S.walk.held = 0; S.walk.end = "chunk limit";
        if (hipMemGetInfo(&fr0, &tot) != hipSuccess) { (void)hipGetLastError(); fr0 = 0; }
        w.hold_cap = std::min(T.hold_max, (size_t)(T.hold_frac * (double)fr0));
        // (one of the three groups is a single stretch of 96 GiB: a matrix whose stream lies in it -- a fresh box hands out that
        //  stretch first -- has its nearest better place up to 96 chunks away.  Timing a chunk costs 2 ms: every fourth is timed up to
        //  the 32nd, every eighth beyond.)
        for (int q = 0; q < T.max_chunks; q++) {
            if (!next_chunk(w, q)) break;
            if (q % (q < 32 ? 4 : 8) != 0) continue;
            if (!look(w)) break;
        }
        if (w.found && std::strcmp(S.walk.end, "chunk limit") == 0) S.walk.end = "found";
        S.walk.ms = w.elapsed();
        S.walk.found = w.found ? 1 : 0;
        if (debug_on()) fprintf(stderr, "[lcg_hip] placement walk: %d chunks of %.0f MiB (%zu given back, %.1f GiB held at most), %s (%.1f us against %.1f), "
                                "%.1f ms of %.0f allowed (allocations %.1f ms, the slowest %.1f), ended by: %s\n", S.walk.chunks, (double)CH / 1048576.0, w.chunks.size(), (double)S.walk.held / 1073741824.0,
                                w.found ? "a faster place found and kept" : "nothing faster", w.found_us, w.ours, S.walk.ms, T.wall_ms, w.alloc_sum, w.alloc_max, S.walk.end);
        for (double *p : w.chunks) { (void)hipFree(p); S.forget_vector(p); S.gave_back(CH); }       // (gave_back site 2)
        if (w.rc && w.found) { (void)hipFree(w.found); S.forget_vector(w.found); S.gave_back(CH); w.found = nullptr; }     // (site 3)
        *found = w.found; *found_us = w.found_us;
        return w.rc;
    }

    // the chunk as an arena of the pool: slots of the vector's size (2 MiB-aligned), as many as the solve has roles + 2
    void keep_as_arena(double *found, float found_us)
    {
        // (two arenas at most: an older one that nobody uses goes first; its slots may stand among the candidates)
        std::vector<double *> gone;
        while (c.pool.evict_idle_arena(gone)) S.gave_back(T.chunk);        // (site 4: the chunk size of NOW)
        for (size_t i = 0; i < cand.size();)
            if (cand[i].role == nullptr && std::find(gone.begin(), gone.end(), cand[i].p) != gone.end()) cand.erase(cand.begin() + (long)i); else i++;
        const size_t slot = (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
        const size_t want = std::min(T.chunk / slot, n_own + 2);
        c.pool.add_arena(found, slot, want);
        for (size_t i = 0; i < want; i++) {
            double *p = reinterpret_cast<double *>(reinterpret_cast<char *>(found) + i * slot);
            if (i > 0) S.memo.push_back({val, p, found_us});
            cand.push_back({nullptr, p, found_us});
        }
    }

    // Every role is dealt, the heaviest first.  (Outputs only -- the vector the product reads pays less beside the values than the output
    // does, and the clock of one product cannot tell the two other groups apart -- was tried after one process in fifteen came out 2.5 %
    // slower placed than as allocated: on a box where nothing allocated is fast it gave 1488-1504 it/s where all roles out of the
    // found arena give 1524-1553; and trial SOLVES of six iterations per assignment, to let the loop itself choose, differ by less
    // than their own order effect.  Both are in profiles/r04_placement.txt; neither is in the code.)
    // Deal the roles by weight: a role keeps its vector unless one that no heavier role holds is clearly faster.  Positions trade
    // vectors, so every role still has a vector of its own; a vector of the pool that lands in a role joins the solve (the one it
    // displaced stays with the solve, unused, and returns to the pool with the others).
    void deal(Workspace &ws)
    {
        for (size_t o = 0; o < n_own; o++) {
            size_t best = o;
            for (size_t j = o + 1; j < cand.size(); j++) if (cand[j].us < cand[best].us) best = j;
            if (best != o && cand[best].us * SAME < cand[o].us) { std::swap(cand[o].p, cand[best].p); std::swap(cand[o].us, cand[best].us); }
        }
        for (size_t i = 0; i < n_own; i++) {
            if (*cand[i].role == cand[i].p) continue;
            *cand[i].role = cand[i].p;
            if (!ws.owns(cand[i].p)) ws.adopt(cand[i].p);
            S.last.moved++;
        }
        S.last.us_chosen = cand[0].us;
    }

    void report() const
    {
        fprintf(stderr, "[lcg_hip] placement: %d timed, %d roles moved; first output %.1f -> %.1f us; roles by weight:", S.last.timed, S.last.moved,
                S.last.us_first, S.last.us_chosen);
        for (size_t i = 0; i < cand.size(); i++) fprintf(stderr, "%s %.1f", i == n_own ? " | idle:" : "", cand[i].us);
        fprintf(stderr, "\n");
    }

    int run(Workspace &ws, std::initializer_list<double **> roles, int n_out)
    {
        if (!candidates(ws, roles, n_out)) return 0;
        bool go = false;
        TRY(gate(&go));
        if (!go) return 0;
        TRY(time_all());
        if (walk_wanted()) {
            double *found = nullptr; float found_us = 0.f;
            TRY(walk(&found, &found_us));
            if (found) keep_as_arena(found, found_us);
            S.memo.push_back({val, nullptr, 0.f});
        }
        deal(ws);
        if (debug_on()) report();
        return 0;
    }
};

} // namespace

// Placement is an optimisation: a timing that fails (an event that cannot be made, a trial product that errors) means
// "not tried" -- the roles stay as allocated (they are dealt only after the last timing) and the solve goes on.
int place_roles(Ctx &c, int n, const void *afp, void *inst, const double *x, Workspace &ws, std::initializer_list<double **> roles, int n_out)
{
    c.place.last = PlaceState::Solve();
    if (!wanted(c, n, afp, inst)) return 0;
    const int rc = Placing(c, n, inst, x).run(ws, roles, n_out);
    if (rc) {
        if (debug_on()) fprintf(stderr, "[lcg_hip] placement: a timing failed (rc %d: %s): not tried, the vectors stay as allocated\n", rc, c.err.c_str());
        (void)hipGetLastError();
        c.place.last.timed = c.place.last.moved = 0;
    }
    return 0;
}

} // namespace lcgh

using namespace lcgh;

extern "C" {

int lcg_hip_trim(void)
{
    Ctx &c = ctx();
    if (!c.inited) return 0;
    (void)hipDeviceSynchronize();
    c.place.gave_back(c.pool.trim());       // (site 1)
    c.place.forget_all();       // (addresses may come back as other memory)
    return 0;
}
int lcg_hip_pool_info(int *vectors, int64_t *bytes, int *arena_slots) { ctx().pool.totals(vectors, bytes, arena_slots); return 0; }
int lcg_hip_pool_add_arena_for_test(uint64_t slot_bytes, int slots)
{
    if (slot_bytes == 0 || slots <= 0) return LCG_HIP_E_ARG;
    int rc = ensure_init(); if (rc) return rc;
    const size_t slot = ((size_t)slot_bytes + 255) & ~(size_t)255;
    void *base = nullptr;
    HIPCHK(hipMalloc(&base, slot * (size_t)slots));
    ctx().pool.add_arena(base, slot, (size_t)slots);
    return 0;
}
int lcg_hip_placement_tune_for_test(uint64_t stream_min_bytes, uint64_t chunk_bytes, int max_chunks, double wall_ms, uint64_t hold_max_bytes,
                                    int force_find_at, int allow_shared)
{
    int rc = ensure_init(); if (rc) return rc;
    PlaceState::Tune t;     // zeros / negatives: the production value
    if (stream_min_bytes) t.stream_min = (size_t)stream_min_bytes;
    if (chunk_bytes) t.chunk = ((size_t)chunk_bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
    if (max_chunks > 0) t.max_chunks = max_chunks;
    if (wall_ms > 0.0) t.wall_ms = wall_ms;
    if (hold_max_bytes) t.hold_max = (size_t)hold_max_bytes;
    t.force_find_at = force_find_at;
    if (allow_shared) t.shared_min = ~(size_t)0;
    if (allow_shared == 1) { t.released_max = ~(size_t)0; t.predict = false; }    // (a test walks many times in one process; 2 keeps the fresh-allocator rule)
    ctx().place.tune = t;
    return 0;
}
int lcg_hip_last_placement_walk(int *chunks, double *wall_ms, int64_t *held_bytes, int *found, const char **ended)
{
    const PlaceState::Walk &w = ctx().place.walk;
    if (chunks) *chunks = w.chunks;
    if (wall_ms) *wall_ms = w.ms;
    if (held_bytes) *held_bytes = (int64_t)w.held;
    if (found) *found = w.found;
    if (ended) *ended = w.end;
    return w.made;
}
int lcg_hip_set_placement(int mode)
{
    if (mode < -1 || mode > 1) return LCG_HIP_E_ARG;
    ctx().place.mode = mode;
    return 0;
}
int lcg_hip_last_placement(int *timed, int *moved, double *us_as_allocated, double *us_as_placed)
{
    const PlaceState::Solve &l = ctx().place.last;
    if (timed) *timed = l.timed;
    if (moved) *moved = l.moved;
    if (us_as_allocated) *us_as_allocated = l.us_first;
    if (us_as_placed) *us_as_placed = l.us_chosen;
    return 0;
}

} // extern "C"
