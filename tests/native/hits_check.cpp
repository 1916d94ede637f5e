// tests/native/hits_check.cpp — CPU checks of the hit table's pure pieces
// (built and run by tests/test_hits_cpu.py):
//   rules     csrc/sw_hits_rules.h's carried-tuple pass (the code sw_hits.hip
//             runs per cell, here in scalar row-major order) against the rows
//             derived from the oracle's traceback (oracle/sw_oracle.c
//             swo_align_linear / swo_align_affine): spans, ops length,
//             identities and positives by replaying the ops over the two
//             sequences, runs of I or of D for gap_opens; and three injected
//             faults, each of which some pair must notice; once over 2 to 4
//             codes (tie-heavy) and once over all 25 codes under asymmetric
//             matrices at the scoring envelope's edges;
//   location  swpack::locate + swk::hit_residue_at against the bytes
//             fill_block / fill_long write: every subject's residues are
//             recovered from its location;
//   groups    swplan::hits_scratch_bytes / hits_groups, and sw_align's swplan::align_dirs_bytes /
//             align_groups.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "sw_hits_rules.h"
#include "sw_kernels.h"
#include "sw_oracle.h"
#include "sw_pack.h"
#include "sw_plan.h"

static int failures = 0;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            if (failures < 20) {               \
                std::printf("FAIL: " __VA_ARGS__); \
                std::printf("\n");             \
            }                                  \
            ++failures;                        \
        }                                      \
    } while (0)

// ---- rules ------------------------------------------------------------------
struct Scoring {
    const char* name;
    std::vector<int8_t> mat;
    int go, ge;
};
struct Pair {
    std::vector<uint8_t> q, s;
};

static bool same_row(const sw_hit& a, const sw_hit& b) {
    return a.score == b.score && a.q_begin == b.q_begin && a.q_end == b.q_end && a.s_begin == b.s_begin &&
           a.s_end == b.s_end && a.length == b.length && a.identities == b.identities && a.positives == b.positives &&
           a.gap_opens == b.gap_opens && a.gaps == b.gaps;
}

// The row the oracle's alignment implies; ops returned for the caller's counts.
static sw_hit oracle_row(const Pair& p, const Scoring& sc, std::string* ops_out) {
    const int qlen = static_cast<int>(p.q.size()), slen = static_cast<int>(p.s.size());
    std::vector<char> ops(static_cast<size_t>(qlen + slen + 1));
    int qe = 0, se = 0, qb = 0, sb = 0, n = 0;
    const int best = sc.go == sc.ge
        ? swo_align_linear(p.q.data(), qlen, p.s.data(), slen, sc.mat.data(), sc.go, &qe, &se, &qb, &sb, ops.data(),
                           static_cast<int>(ops.size()), &n)
        : swo_align_affine(p.q.data(), qlen, p.s.data(), slen, sc.mat.data(), sc.go, sc.ge, &qe, &se, &qb, &sb,
                           ops.data(), static_cast<int>(ops.size()), &n);
    sw_hit r;
    std::memset(&r, 0, sizeof r);
    ops_out->assign(ops.data(), static_cast<size_t>(n));
    if (best <= 0) return r;  // the score-0 normalisation: every field 0
    r.score = best;
    r.q_begin = qb; r.q_end = qe; r.s_begin = sb; r.s_end = se;
    r.length = n;
    int i = qb - 1, j = sb - 1;
    char prev = 0;
    for (int k = 0; k < n; ++k) {
        const char op = ops[k];
        if (op == 'M') {
            r.identities += p.q[i] == p.s[j];
            r.positives += sc.mat[25 * p.q[i] + p.s[j]] > 0;
            ++i; ++j;
        } else {
            r.gaps += 1;
            r.gap_opens += op != prev;
            if (op == 'I') ++i; else ++j;
        }
        prev = op;
    }
    CHECK(i == qe && j == se, "%s: the oracle's path does not end at its end cell", sc.name);
    return r;
}

template <int FAULT>
static sw_hit carried_row(const Pair& p, const Scoring& sc) {
    sw_hit r;
    std::memset(&r, 0, sizeof r);
    swhits::scalar_pass<FAULT>(p.q.data(), static_cast<int32_t>(p.q.size()), p.s.data(), static_cast<int32_t>(p.s.size()),
                               sc.mat.data(), sc.go, sc.ge, r);
    return r;
}

// Every pair under every scoring: the carried row equals the oracle's; the
// counts printed under `tag` are what tests/test_hits_cpu.py asserts.
static void run_rules(const char* tag, const std::vector<Scoring>& scorings, const std::vector<Pair>& pairs, int at_least) {
    int total = 0, gapped = 0, adjacent = 0, zero = 0, id_over_pos = 0, pos_over_id = 0, big = 0, caught[4] = {};
    for (const Scoring& sc : scorings)
        for (const Pair& p : pairs) {
            std::string ops;
            const sw_hit want = oracle_row(p, sc, &ops);
            const sw_hit got = carried_row<swhits::kFaultNone>(p, sc);
            ++total;
            gapped += want.gaps > 0;
            adjacent += ops.find("ID") != std::string::npos || ops.find("DI") != std::string::npos;
            zero += want.score == 0;
            id_over_pos += want.identities > want.positives;
            pos_over_id += want.positives > want.identities;
            big += want.score > 32767;
            CHECK(same_row(got, want),
                  "%s pair %d: carried %d [%d,%d]x[%d,%d] len %d id %d pos %d opens %d gaps %d, oracle %d [%d,%d]x[%d,%d] "
                  "len %d id %d pos %d opens %d gaps %d (%s)",
                  sc.name, total, got.score, got.q_begin, got.q_end, got.s_begin, got.s_end, got.length, got.identities,
                  got.positives, got.gap_opens, got.gaps, want.score, want.q_begin, want.q_end, want.s_begin, want.s_end,
                  want.length, want.identities, want.positives, want.gap_opens, want.gaps, ops.c_str());
            caught[1] += !same_row(carried_row<swhits::kFaultLastOp>(p, sc), want);
            caught[2] += !same_row(carried_row<swhits::kFaultTieBegin>(p, sc), want);
            caught[3] += !same_row(carried_row<swhits::kFaultPositives>(p, sc), want);
        }
    CHECK(total >= at_least, "only %d pairs", total);
    CHECK(3 * gapped >= total, "only %d of %d alignments contain a gap", gapped, total);
    CHECK(adjacent > 0, "no alignment has adjacent I and D runs");
    CHECK(caught[1] > 0, "no pair notices a last op dropped at a source change");
    CHECK(caught[2] > 0, "no pair notices a begin cell taken from the losing source of a tie");
    CHECK(caught[3] > 0, "no pair notices positives counted on entries >= 0");
    std::printf("%s: %d pairs, %d gapped, %d adjacent-runs, %d score-0, faults caught %d %d %d\n", tag, total, gapped,
                adjacent, zero, caught[1], caught[2], caught[3]);
    std::printf("%s-counts: %d identities-over-positives, %d positives-over-identities, %d over-16-bits\n", tag, id_over_pos,
                pos_over_id, big);
}

static void check_rules() {
    std::mt19937 rng(20261);
    auto rnd = [&](int lo, int hi) { return lo + static_cast<int>(rng() % static_cast<unsigned>(hi - lo + 1)); };
    std::vector<Scoring> scorings;
    auto builtin = [](int id) { const int8_t* m = swo_matrix(id); return std::vector<int8_t>(m, m + 625); };
    scorings.push_back({"identity3-gap2", builtin(2), 2, 2});
    scorings.push_back({"blosum62-11-1", builtin(1), 11, 1});
    scorings.push_back({"blosum62-12-1", builtin(1), 12, 1});
    scorings.push_back({"identity3-open-below-extend", builtin(2), 2, 3});
    scorings.push_back({"identity3-affine-3-1", builtin(2), 3, 1});
    {
        std::vector<int8_t> m(625);
        for (auto& v : m) v = static_cast<int8_t>(rnd(-4, 5));
        bool asym = false;
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < a; ++b) asym |= m[25 * a + b] != m[25 * b + a];
        CHECK(asym, "the random matrix is symmetric over the codes used");
        scorings.push_back({"asymmetric-3-1", m, 3, 1});
    }
    constexpr int kPairsPerScoring = 500;
    std::vector<Pair> pairs;
    for (int k = 0; k < kPairsPerScoring; ++k) {
        const int alpha = rnd(2, 4);
        Pair p;
        p.q.resize(static_cast<size_t>(rnd(1, 60)));
        for (auto& c : p.q) c = static_cast<uint8_t>(rnd(0, alpha - 1));
        if (k % 4 == 0) {  // unrelated
            p.s.resize(static_cast<size_t>(rnd(1, 60)));
            for (auto& c : p.s) c = static_cast<uint8_t>(rnd(0, alpha - 1));
        } else {  // a copy with deletions, insertions and substitutions
            p.s = p.q;
            for (int e = rnd(1, 3); e > 0 && !p.s.empty(); --e) {
                const size_t at = static_cast<size_t>(rnd(0, static_cast<int>(p.s.size()) - 1));
                const int L = rnd(1, 4);
                if (rnd(0, 1)) {
                    p.s.erase(p.s.begin() + at, p.s.begin() + std::min(p.s.size(), at + L));
                } else {
                    std::vector<uint8_t> ins(static_cast<size_t>(L));
                    for (auto& c : ins) c = static_cast<uint8_t>(rnd(0, alpha - 1));
                    p.s.insert(p.s.begin() + at, ins.begin(), ins.end());
                }
            }
            for (int e = rnd(0, 2); e > 0 && !p.s.empty(); --e)
                p.s[static_cast<size_t>(rnd(0, static_cast<int>(p.s.size()) - 1))] = static_cast<uint8_t>(rnd(0, alpha - 1));
            if (p.s.empty()) p.s.push_back(0);
            if (p.s.size() > 60) p.s.resize(60);
        }
        pairs.push_back(p);
    }
    run_rules("rules", scorings, pairs, 2000);
}

// The same pass over all 25 codes (B, J, Z, X and * included) under matrices
// that are not symmetric: entries -12..12 with a positive diagonal (asym), the
// same with three diagonal entries <= 0 (idneg: identities that are not
// positives) and entries of +-100 (pm100); gaps from 1 to 1000 and an open
// below the extend; sequences up to 200 residues.  A rules error at the
// envelope's edges shows here, on the CPU; tests/test_gpu_hits_envelope.py is
// left to find the kernel's own (profile, hand-overs, reduction).
static void check_rules25() {
    std::mt19937 rng(20262);
    auto rnd = [&](int lo, int hi) { return lo + static_cast<int>(rng() % static_cast<unsigned>(hi - lo + 1)); };
    auto asymmetric = [](const std::vector<int8_t>& m) {
        int n = 0;
        for (int a = 0; a < 25; ++a)
            for (int b = 0; b < a; ++b) n += m[25 * a + b] != m[25 * b + a];
        return n;
    };
    std::vector<int8_t> asym(625), pm100(625);
    for (auto& v : asym) v = static_cast<int8_t>(rnd(-12, 12));
    for (int a = 0; a < 25; ++a) asym[26 * a] = static_cast<int8_t>(rnd(3, 13));
    std::vector<int8_t> idneg = asym;
    idneg[26 * 4] = 0;
    idneg[26 * 21] = -2;
    idneg[26 * 23] = 0;
    for (auto& v : pm100) v = rnd(0, 9) < 3 ? 100 : -100;
    for (int a = 0; a < 24; ++a) pm100[26 * a] = 100;
    pm100[26 * 24] = -100;
    CHECK(asymmetric(asym) > 100 && asymmetric(idneg) > 100 && asymmetric(pm100) > 50,
          "a 25-code matrix is (nearly) symmetric: %d %d %d", asymmetric(asym), asymmetric(idneg), asymmetric(pm100));
    std::vector<Scoring> scorings;
    scorings.push_back({"asym-12-1", asym, 12, 1});
    scorings.push_back({"asym-2-2", asym, 2, 2});
    scorings.push_back({"asym-1-4-open-below-extend", asym, 1, 4});
    scorings.push_back({"idneg-11-1", idneg, 11, 1});
    scorings.push_back({"pm100-1000-1000", pm100, 1000, 1000});
    scorings.push_back({"pm100-3-1", pm100, 3, 1});
    constexpr int kPairs = 260;
    std::vector<Pair> pairs;
    bool seen_q[25] = {}, seen_s[25] = {};
    for (int k = 0; k < kPairs; ++k) {
        Pair p;
        p.q.resize(static_cast<size_t>(k % 5 == 0 ? rnd(150, 200) : rnd(1, 200)));
        for (auto& c : p.q) c = static_cast<uint8_t>(rnd(0, 24));
        if (k % 3 == 0) {  // unrelated
            p.s.resize(static_cast<size_t>(rnd(1, 200)));
            for (auto& c : p.s) c = static_cast<uint8_t>(rnd(0, 24));
        } else {  // a copy with deletions, insertions and substitutions
            p.s = p.q;
            for (int e = rnd(1, 4); e > 0 && !p.s.empty(); --e) {
                const size_t at = static_cast<size_t>(rnd(0, static_cast<int>(p.s.size()) - 1));
                const int L = rnd(1, 5);
                if (rnd(0, 1)) {
                    p.s.erase(p.s.begin() + at, p.s.begin() + std::min(p.s.size(), at + L));
                } else {
                    std::vector<uint8_t> ins(static_cast<size_t>(L));
                    for (auto& c : ins) c = static_cast<uint8_t>(rnd(0, 24));
                    p.s.insert(p.s.begin() + at, ins.begin(), ins.end());
                }
            }
            for (int e = rnd(0, 6); e > 0 && !p.s.empty(); --e)
                p.s[static_cast<size_t>(rnd(0, static_cast<int>(p.s.size()) - 1))] = static_cast<uint8_t>(rnd(0, 24));
            if (p.s.empty()) p.s.push_back(24);
            if (p.s.size() > 200) p.s.resize(200);
        }
        for (const uint8_t c : p.q) seen_q[c] = true;
        for (const uint8_t c : p.s) seen_s[c] = true;
        pairs.push_back(p);
    }
    for (int c = 0; c < 25; ++c) CHECK(seen_q[c] && seen_s[c], "code %d is in no query or in no subject", c);
    run_rules("rules25", scorings, pairs, 1500);
}

// ---- location ---------------------------------------------------------------
static void check_location(int64_t n, int32_t threshold, const char* tname) {
    static const int64_t kLens[] = {15, 16, 17, 1, 0, 33, 100, 31, 32, 64, 65, 48};
    std::vector<int64_t> offs(static_cast<size_t>(n) + 1, 0);
    for (int64_t k = 0; k < n; ++k) offs[k + 1] = offs[k] + kLens[k % 12];
    std::vector<int32_t> ids(static_cast<size_t>(n));
    for (int64_t k = 0; k < n; ++k) ids[k] = static_cast<int32_t>(3 * k + 1);
    std::vector<uint8_t> res(static_cast<size_t>(offs[n]) + 1);
    for (int64_t k = 0; k < n; ++k)
        for (int64_t j = 0; j < offs[k + 1] - offs[k]; ++j) res[offs[k] + j] = static_cast<uint8_t>((7 * k + 3 * j + 2) % 25);
    swpack::Subjects subj;
    subj.n = n;
    subj.offsets = offs.data();
    subj.ids = ids.data();
    subj.residues = res.data();
    if (threshold < 0) {
        swplan::PlanDb v;
        v.n = n;
        v.residues = offs[n];
        threshold = swplan::default_long_threshold(v);
    }
    const swpack::Shape sh = swpack::plan(subj, threshold, false);
    // the database's bytes, as build_db uploads them
    std::vector<uint8_t> inter(sh.total + 1, 0xee), longs(sh.ltotal + 1, 0xee);
    for (int64_t b = 0; b < sh.nblocks; ++b) swpack::fill_block(subj, sh, b, inter.data() + sh.blk_off[b]);
    for (int64_t k = 0; k < sh.nlong; ++k) swpack::fill_long(subj, sh, k, longs.data() + sh.loff[k]);
    // position of each subject: what sw_db.cpp's position_of rebuilds from length_order
    const std::vector<int64_t> order = swpack::length_order(offs.data(), n);
    int64_t recovered = 0;
    for (int64_t p = 0; p < n; ++p) {
        const int64_t k = order[p], L = offs[k + 1] - offs[k];
        const swpack::Location loc = swpack::locate(p, sh.nlong);
        CHECK((loc.lane < 0) == (p < sh.nlong), "%lld/%s: position %lld on the wrong side", (long long)n, tname, (long long)p);
        const bool is_long = loc.lane < 0;
        CHECK(loc.slot >= 0 && loc.slot < (is_long ? sh.nlong : sh.nblocks) && loc.lane < swk::kLanes,
              "%lld/%s: position %lld: slot %lld lane %d out of range", (long long)n, tname, (long long)p,
              (long long)loc.slot, loc.lane);
        if (!is_long) CHECK(sh.lane_ids[loc.slot * swk::kLanes + loc.lane] == ids[k], "%lld/%s: lane id", (long long)n, tname);
        else CHECK(sh.lid[loc.slot] == ids[k] && sh.llen[loc.slot] == L, "%lld/%s: long id", (long long)n, tname);
        const uint8_t* base = is_long ? longs.data() + sh.loff[loc.slot] : inter.data() + sh.blk_off[loc.slot];
        const uint64_t room = is_long ? sh.loff[loc.slot + 1] - sh.loff[loc.slot]
                                      : static_cast<uint64_t>(sh.blk_groups[loc.slot]) * swk::kGroupBytes;
        bool ok = true;
        for (int64_t j = 0; j < L; ++j) {
            const uint64_t at = swk::hit_residue_at(loc.lane, static_cast<uint64_t>(j));
            ok = ok && at < room && swk::kCodeOf[base[at]] == res[offs[k] + j];
        }
        CHECK(ok, "%lld/%s: subject %lld (length %lld) is not at slot %lld lane %d", (long long)n, tname, (long long)k,
              (long long)L, (long long)loc.slot, loc.lane);
        recovered += ok;
    }
    std::printf("location-n%lld-%s: %lld recovered, %lld long, %lld blocks\n", (long long)n, tname, (long long)recovered,
                (long long)sh.nlong, (long long)sh.nblocks);
}

// ---- groups -------------------------------------------------------------------
static void check_groups() {
    const int C = swk::kHitsChunkRows;
    CHECK(swplan::hits_scratch_bytes(C, 1000) == 0 && swplan::hits_scratch_bytes(1, 1000) == 0 &&
              swplan::hits_scratch_bytes(0, 1000) == 0,
          "a query of one chunk needs no scratch");
    const int64_t per = swplan::hits_scratch_bytes(C + 1, 1);
    CHECK(per == swk::kHitsBndWords * 4, "bytes per column");
    for (int q : {C + 1, 2 * C, 10 * C + 3, 1 << 20})
        for (int64_t s : {int64_t(0), int64_t(1), int64_t(17), int64_t(35213), int64_t(1) << 30})
            CHECK(swplan::hits_scratch_bytes(q, s) == per * s, "scratch is proportional to slen alone (q %d)", q);
    std::mt19937 rng(7);
    for (int round = 0; round < 50; ++round) {
        const int64_t n = rng() % 40;
        const int64_t budget = per * (1 + rng() % 2000);
        std::vector<int64_t> slens(static_cast<size_t>(n));
        for (auto& s : slens) s = rng() % 10 == 0 ? 3000 + rng() % 3000 : rng() % 700;  // some alone over the budget
        for (int q : {C, C + 1}) {
            const std::vector<int64_t> ends = swplan::hits_groups(q, slens.data(), n, budget);
            CHECK((n == 0) == ends.empty() && (n == 0 || ends.back() == n), "groups end at n");
            int64_t k0 = 0;
            for (const int64_t k1 : ends) {
                CHECK(k1 > k0, "an empty group");
                int64_t bytes = 0;
                for (int64_t k = k0; k < k1; ++k) bytes += swplan::hits_scratch_bytes(q, slens[k]);
                CHECK(bytes <= budget || k1 == k0 + 1, "a group of %lld hits holds %lld bytes, budget %lld",
                      (long long)(k1 - k0), (long long)bytes, (long long)budget);
                // greedy: the next hit would not have fitted
                if (k1 < n) CHECK(bytes + swplan::hits_scratch_bytes(q, slens[k1]) > budget, "a group closed early");
                k0 = k1;
            }
            if (q == C) CHECK(ends.size() <= 1, "no scratch, one group");
        }
    }
    const int64_t big[3] = {10, (int64_t(1) << 30) / per + 1, 10};
    const std::vector<int64_t> ends = swplan::hits_groups(C + 1, big, 3);
    CHECK(ends.size() == 3 && ends[0] == 1 && ends[1] == 2 && ends[2] == 3, "an over-budget hit forms its own group");
    std::printf("groups: %lld bytes per column\n", (long long)per);
}

// ---- sw_align's groups -----------------------------------------------------------
static void check_align_groups() {
    CHECK(swplan::align_dirs_bytes(0, 0) == 1 && swplan::align_dirs_bytes(3, 5) == 9 * 4 &&
              swplan::align_dirs_bytes(16383, 16385) == 536887296,
          "(qlen + slen + 1) (qlen + 1) bytes per hit");
    CHECK(swplan::align_dirs_bytes(1 << 20, int64_t(1) << 30) == ((int64_t(1) << 30) + (1 << 20) + 1) * ((1 << 20) + 1),
          "64-bit sizes");
    std::mt19937 rng(11);
    int64_t multi = 0, alone = 0;
    for (int round = 0; round < 200; ++round) {
        const int64_t n = rng() % 40;
        const int32_t q = 1 + rng() % 300;
        const int64_t budget = swplan::align_dirs_bytes(q, 1 + rng() % 2000);
        std::vector<int64_t> slens(static_cast<size_t>(n));
        for (auto& s : slens) s = rng() % 10 == 0 ? 3000 + rng() % 3000 : rng() % 700;  // some alone over the budget
        const std::vector<int64_t> ends = swplan::align_groups(q, slens.data(), n, budget);
        CHECK((n == 0) == ends.empty() && (n == 0 || ends.back() == n), "align groups end at n");
        int64_t k0 = 0;
        for (const int64_t k1 : ends) {  // the groups tile [0, n) in order
            CHECK(k1 > k0, "an empty align group");
            int64_t bytes = 0;
            for (int64_t k = k0; k < k1; ++k) bytes += swplan::align_dirs_bytes(q, slens[k]);
            CHECK(bytes <= budget || k1 == k0 + 1, "an align group of %lld hits holds %lld bytes, budget %lld",
                  (long long)(k1 - k0), (long long)bytes, (long long)budget);
            // greedy: the next hit would not have fitted
            if (k1 < n) CHECK(bytes + swplan::align_dirs_bytes(q, slens[k1]) > budget, "an align group closed early");
            multi += k1 > k0 + 1;
            alone += bytes > budget;
            k0 = k1;
        }
    }
    CHECK(multi > 100 && alone > 100, "the rounds reach groups of several hits (%lld) and over-budget hits (%lld)",
          (long long)multi, (long long)alone);
    // the exact fit: hits that fill the budget to the byte stay together, one byte less splits them
    const int64_t fit[3] = {7, 12, 30};
    const int64_t exact = swplan::align_dirs_bytes(9, 7) + swplan::align_dirs_bytes(9, 12) + swplan::align_dirs_bytes(9, 30);
    std::vector<int64_t> ends = swplan::align_groups(9, fit, 3, exact);
    CHECK(ends.size() == 1 && ends[0] == 3, "an exact fit is one group");
    ends = swplan::align_groups(9, fit, 3, exact - 1);
    CHECK(ends.size() == 2 && ends[0] == 2 && ends[1] == 3, "one byte under the exact fit splits before the last hit");
    // a query of 16,383 against 16,385, 16,385 and 100 residues at the default budget: each of the
    // long hits takes just over half of it
    const int64_t three[3] = {16385, 16385, 100};
    CHECK(2 * swplan::align_dirs_bytes(16383, 16385) > swplan::kAlignDirsBudget &&
              swplan::align_dirs_bytes(16383, 16385) + swplan::align_dirs_bytes(16383, 100) <= swplan::kAlignDirsBudget,
          "the three-hit case straddles the default budget");
    ends = swplan::align_groups(16383, three, 3);
    CHECK(ends.size() == 2 && ends[0] == 1 && ends[1] == 3, "the three-hit case groups as {0}, {1, 2}");
    std::printf("align_groups: budget %lld, three-hit ends %lld %lld\n", (long long)swplan::kAlignDirsBudget,
                ends.size() == 2 ? (long long)ends[0] : -1LL, ends.size() == 2 ? (long long)ends[1] : -1LL);
}

int main() {
    check_rules();
    check_rules25();
    for (int64_t n : {0, 1, 63, 64, 65, 129}) {
        check_location(n, 0, "all-long");
        check_location(n, 16, "t16");
        check_location(n, 64, "t64");
        check_location(n, 1000, "none-long");
        check_location(n, -1, "default");
    }
    check_groups();
    check_align_groups();
    std::printf("chunk_rows: %d\n", swk::kHitsChunkRows);
    std::printf("rows_per_lane: %d\nwaves: %d\n", swk::kHitsRowsPerLane, swk::kHitsWaves);
    std::printf(failures ? "hits_check FAILED (%d)\n" : "hits_check ok\n", failures);
    return failures ? 1 : 0;
}
