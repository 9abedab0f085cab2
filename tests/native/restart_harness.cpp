// CPU harness for the store half of the stream restart (uav_airvision_amd/csrc/msckf_store.h: avs_restart, the function dk_restart
// calls, compiled here with a one-thread team: AVS_CPU_MODEL).  A store is driven through a random message sequence -- the operations of a
// filter step in a step's order: add_frame, select_lost, erase, and with a full window select_prune and two remove_frame -- until frame
// slots, the feature table, the free stack and the insertion counter are all in use; the header's overflow word and its spare words are
// set by hand (no operation writes them; the restart must not depend on that).  Then avs_restart is applied and
//   check one: every persistent array of the store equals that of a store as it is first allocated (zero, pos_of / order -1);
//   check two: a second random sequence replayed into both leaves identical persistent arrays and identical results after every frame.
// avs_clear alone -- the online reset -- is shown NOT to pass check one (the insertion counter and the overflow word stay).
// Run under ASan / UBSan.  Arguments: seed, frames before the restart, frames after it, features per frame.
#define AVS_CPU_MODEL 1
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "msckf_store.h"

struct Owned {
    std::vector<long long> fr_id, births, m_id, m_birth; std::vector<double> fr_z, m_pos;
    std::vector<int> fr_fslot, fr_prev, fr_next, fr_n, pos_of, order, hdr, m_init, m_nobs, m_tail, free_stack, ha, hb, hc, ta, tb, tc;
    std::vector<unsigned long long> keys;
    AvsStore V;
    // as dev_reserve allocates it: every array zero, pos_of / order filled with 0xFF bytes; the scratch arrays get a pattern of their
    // own per store (`junk`), so that a result that depended on them would differ between two stores
    Owned(int cap, int ns, int junk)
    {
        V.cap = cap; V.mcap = 2 * cap + 64; V.ns = ns;
        int hc_ = 64; while (hc_ < 2 * cap + 16) hc_ *= 2;
        V.hcells = hc_;
        fr_id.assign((size_t)ns * cap, 0); fr_z.assign((size_t)ns * cap * 4, 0.0); fr_fslot.assign((size_t)ns * cap, 0); fr_prev.assign((size_t)ns * cap, 0); fr_next.assign((size_t)ns * cap, 0);
        fr_n.assign(ns, 0); pos_of.assign(ns, -1); order.assign(ns, -1); hdr.assign(AVS_HDR_WORDS, 0); births.assign(1, 0);
        m_id.assign(V.mcap, 0); m_birth.assign(V.mcap, 0); m_pos.assign((size_t)V.mcap * 3, 0.0); m_init.assign(V.mcap, 0); m_nobs.assign(V.mcap, 0); m_tail.assign(V.mcap, 0); free_stack.assign(V.mcap, 0);
        ha.assign(hc_, junk); hb.assign(hc_, junk); hc.assign(hc_, junk); ta.assign(cap, junk); tb.assign(cap, junk); tc.assign(cap, junk); keys.assign(cap, (unsigned long long)junk);
        V.fr_id = fr_id.data(); V.fr_z = fr_z.data(); V.fr_fslot = fr_fslot.data(); V.fr_prev = fr_prev.data(); V.fr_next = fr_next.data();
        V.fr_n = fr_n.data(); V.pos_of = pos_of.data(); V.order = order.data(); V.hdr = hdr.data(); V.births = births.data();
        V.m_id = m_id.data(); V.m_birth = m_birth.data(); V.m_pos = m_pos.data(); V.m_init = m_init.data(); V.m_nobs = m_nobs.data(); V.m_tail = m_tail.data();
        V.free_stack = free_stack.data(); V.hash_a = ha.data(); V.hash_b = hb.data(); V.hash_c = hc.data(); V.tmp_a = ta.data(); V.tmp_b = tb.data(); V.tmp_c = tc.data(); V.keys = keys.data();
    }
};

template <typename T>
static bool eq(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T))); }

// the name of the first persistent array that differs, or null
static const char* differs(const Owned& a, const Owned& b)
{
#define C(f) if (!eq(a.f, b.f)) return #f;
    C(fr_id) C(fr_z) C(fr_fslot) C(fr_prev) C(fr_next) C(fr_n) C(pos_of) C(order) C(hdr) C(births)
    C(m_id) C(m_birth) C(m_pos) C(m_init) C(m_nobs) C(m_tail) C(free_stack)
#undef C
    return nullptr;
}

// messages of a run: independent of any store (the window's size follows from the frame count alone)
struct Gen {
    std::mt19937 rng; long long next_id = 1; std::vector<long long> alive; int window = 0, per, cap, max_cam;
    Gen(unsigned seed, int per_, int cap_, int max_cam_) : rng(seed), per(per_), cap(cap_), max_cam(max_cam_) {}
    struct Msg { std::vector<long long> ids; std::vector<double> uv; int i0 = -1, i1 = -1; };
    Msg next()
    {
        Msg m;
        for (long long id : alive) if (rng() % 100 < 85) m.ids.push_back(id);
        std::shuffle(m.ids.begin(), m.ids.end(), rng);
        const int room = per - (int)m.ids.size();
        const int n_new = room > 0 ? (int)(rng() % (unsigned)(room + 1)) : 0;
        for (int k = 0; k < n_new; ++k) m.ids.push_back(next_id++);
        if (!m.ids.empty() && rng() % 7 == 0) m.ids.push_back(m.ids[rng() % m.ids.size()]);          // a duplicate id now and then
        if (rng() % 31 == 0) m.ids.clear();                  // a blank frame loses every track
        if ((int)m.ids.size() > cap) m.ids.resize(cap);
        m.uv.resize(4 * m.ids.size());
        for (double& v : m.uv) v = (double)(rng() % 100000) / 1000.0;
        alive = m.ids;                                       // what is not in this message is lost with it
        std::sort(alive.begin(), alive.end()); alive.erase(std::unique(alive.begin(), alive.end()), alive.end());
        ++window;
        if (window >= max_cam) {
            m.i0 = (int)(rng() % (unsigned)(window - 1)); m.i1 = (int)(rng() % (unsigned)(window - 1));
            if (m.i0 == m.i1) m.i1 = (m.i0 + 1) % (window - 1);
            if (m.i0 > m.i1) std::swap(m.i0, m.i1);
            window -= 2;
        }
        return m;
    }
};

// one step's store operations; what they returned, for the comparison of two stores
struct Result { int slot, tracked, nc, ni, np; std::vector<int> cand, inval, pc, e0, e1; };
static bool apply(Owned& O, const Gen::Msg& m, Result* r)
{
    AvsStore& S = O.V;
    AvsTeam T;
    const int cap = S.cap;
    r->cand.assign(cap, 0); r->inval.assign(cap, 0); r->pc.assign(cap, 0); r->e0.assign(cap, 0); r->e1.assign(cap, 0);
    r->tracked = -1; r->nc = r->ni = 0; r->np = -1;
    r->slot = avs_add_frame(T, S, m.ids.data(), m.uv.data(), (int)m.ids.size(), &r->tracked);
    if (r->slot < 0) return false;
    avs_select_lost(T, S, r->cand.data(), &r->nc, r->inval.data(), &r->ni);
    avs_erase(T, S, r->cand.data(), r->nc);
    avs_erase(T, S, r->inval.data(), r->ni);
    if (m.i0 >= 0) {
        avs_select_prune(T, S, m.i0, m.i1, r->pc.data(), r->e0.data(), r->e1.data(), &r->np);
        avs_remove_frame(T, S, m.i1); avs_remove_frame(T, S, m.i0);
    }
    r->cand.resize(r->nc); r->inval.resize(r->ni); r->pc.resize(r->np < 0 ? 0 : r->np); r->e0.resize(r->pc.size()); r->e1.resize(r->pc.size());
    return true;
}

int main(int argc, char** argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
    const int before = argc > 2 ? atoi(argv[2]) : 60, after = argc > 3 ? atoi(argv[3]) : 80, per = argc > 4 ? atoi(argv[4]) : 40, max_cam = 20;
    const int cap = per + 8, ns = max_cam + 2;
    long long checks = 0;
    Owned U(cap, ns, 0x11111111), F(cap, ns, 0x22222222);
    if (differs(U, F)) { printf("FAIL two new stores differ in %s\n", differs(U, F)); return 1; }
    // ---- a first life, until everything is in use
    Gen g1(seed, per, cap, max_cam);
    Result r;
    const AvsStore& S = U.V;
    auto in_use = [&] { return S.hdr[AVS_N_ORDER] > 0 && S.hdr[AVS_N_FREE] > 0 && S.hdr[AVS_N_USED] > 0 && S.hdr[AVS_LIVE] > 0 && *S.births > 0; };
    // (at least `before` frames; a few more if the last one was a blank frame, which leaves no live feature)
    for (int t = 0; t < before || (!in_use() && t < before + 40); ++t) if (!apply(U, g1.next(), &r)) { printf("FAIL add_frame %d in the first life, frame %d\n", r.slot, t); return 1; }
    if (!in_use()) {
        printf("FAIL the first life left something unused: order %d free %d used %d live %d births %lld\n", S.hdr[AVS_N_ORDER], S.hdr[AVS_N_FREE], S.hdr[AVS_N_USED], S.hdr[AVS_LIVE], *S.births);
        return 1;
    }
    for (int i = AVS_OVERFLOW; i < AVS_HDR_WORDS; ++i) U.hdr[i] = 1 + i;          // the sticky word and the spare ones
    // ---- the online reset is not a restart
    {
        Owned K2(cap, ns, 0x33333333);                       // a copy of the used store, element by element into K2's own buffers
#define CP(f) std::copy(U.f.begin(), U.f.end(), K2.f.begin());
        CP(fr_id) CP(fr_z) CP(fr_fslot) CP(fr_prev) CP(fr_next) CP(fr_n) CP(pos_of) CP(order) CP(hdr) CP(births)
        CP(m_id) CP(m_birth) CP(m_pos) CP(m_init) CP(m_nobs) CP(m_tail) CP(free_stack)
#undef CP
        AvsTeam T;
        avs_clear(T, K2.V);
        if (K2.births[0] == 0 || K2.hdr[AVS_OVERFLOW] == 0) { printf("FAIL avs_clear is expected to leave births and the overflow word\n"); return 1; }
        if (!differs(K2, F)) { printf("FAIL avs_clear alone passes check one: the check has no teeth\n"); return 1; }
        ++checks;
    }
    // ---- the restart
    { AvsTeam T; avs_restart(T, U.V); }
    if (const char* w = differs(U, F)) { printf("FAIL check one: %s differs from a new store\n", w); return 1; }
    checks += 17;
    // ---- a second life, replayed into both
    Gen g2(seed * 7919u + 13u, per, cap, max_cam);
    Result ru, rf;
    bool grew = false;
    for (int t = 0; t < after; ++t) {
        const Gen::Msg m = g2.next();
        const bool au = apply(U, m, &ru), af = apply(F, m, &rf);
        if (!au || !af) { printf("FAIL add_frame %d / %d in the second life, frame %d\n", ru.slot, rf.slot, t); return 1; }
        if (ru.slot != rf.slot || ru.tracked != rf.tracked || ru.nc != rf.nc || ru.ni != rf.ni || ru.np != rf.np || ru.cand != rf.cand || ru.inval != rf.inval ||
            ru.pc != rf.pc || ru.e0 != rf.e0 || ru.e1 != rf.e1) { printf("FAIL check two: results differ at frame %d\n", t); return 1; }
        if (const char* w = differs(U, F)) { printf("FAIL check two: %s differs at frame %d\n", w, t); return 1; }
        checks += 18;
        grew = grew || (F.hdr[AVS_N_FREE] > 0 && m.i0 >= 0);
    }
    if (!grew || F.births[0] == 0) { printf("FAIL the second life never pruned with a free stack in use\n"); return 1; }
    printf("OK %lld checks\n", checks);
    return 0;
}
