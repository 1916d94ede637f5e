// owned_check.cpp — swk::Owned (csrc/sw_owned.h) on the CPU, no HIP: the
// release function runs exactly once per owned value, whatever the owner
// went through (tests/test_owned.py builds and runs this with g++).
#include <cstdio>
#include <map>
#include <utility>
#include <vector>

#include "sw_owned.h"

namespace {

std::map<int, int> g_released;  // value -> times released
int g_fail = 0;

void count(int v) { ++g_released[v]; }
using Tok = swk::Owned<int, count>;  // 0 is the empty value

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s is false\n", __LINE__, #cond);      \
            ++g_fail;                                                    \
        }                                                                \
    } while (0)

int times(int v) { return g_released.count(v) ? g_released[v] : 0; }

// Every value in [lo, hi] was released exactly once.
bool once_each(int lo, int hi) {
    for (int v = lo; v <= hi; ++v)
        if (times(v) != 1) return false;
    return true;
}

// A member-wise movable aggregate of owners, as sw_db::Layout and ScanEvents.
struct Pair {
    Tok a, b[2];
    int plain = 0;
};

}  // namespace

int main() {
    {  // an empty owner releases nothing, at reset() or at its end
        Tok e;
        CHECK(e.get() == 0);
        e.reset();
        CHECK(e.release() == 0);
    }
    CHECK(g_released.empty());

    {  // scope end; reset() releases now and only once
        Tok a(1), b(2);
        CHECK(a.get() == 1);
        b.reset();
        CHECK(times(2) == 1 && b.get() == 0);
        b.reset();
    }
    CHECK(once_each(1, 2));

    {  // release() gives the value up: the owner's end does not release it
        Tok a(3);
        CHECK(a.release() == 3 && a.get() == 0);
    }
    CHECK(times(3) == 0);

    {  // move construction: the source is empty, the value released once
        Tok a(4);
        Tok b(std::move(a));
        CHECK(a.get() == 0 && b.get() == 4 && times(4) == 0);
    }
    CHECK(times(4) == 1);

    {  // move assignment onto an occupied owner releases the old value first
        Tok a(5), b(6);
        a = std::move(b);
        CHECK(times(5) == 1 && times(6) == 0 && a.get() == 6 && b.get() == 0);
        a = Tok();  // onto an occupied owner from an empty one
        CHECK(times(6) == 1 && a.get() == 0);
    }
    CHECK(once_each(5, 6));

    {  // self-move-assignment keeps the value
        Tok a(7);
        Tok& same = a;
        a = std::move(same);
        CHECK(a.get() == 7 && times(7) == 0);
    }
    CHECK(times(7) == 1);

    {  // a vector that reallocates while it grows and erases its front
       // element (sw_handle::evpool, sw_db::Layout::lpt_tables)
        std::vector<Tok> v;
        for (int k = 100; k < 140; ++k) v.emplace_back(k);  // from capacity 0: several reallocations
        CHECK(g_released.count(100) == 0 && times(139) == 0);
        v.erase(v.begin());
        CHECK(times(100) == 1 && v.front().get() == 101 && v.size() == 39);
        for (int k = 101; k < 140; ++k) CHECK(times(k) == 0);
        v.erase(v.begin());
        CHECK(times(101) == 1 && v.front().get() == 102);
    }
    CHECK(once_each(100, 139));

    {  // an aggregate of owners replaced by a fresh one (free_dev), in a vector too
        Pair p{Tok(200), {Tok(201), Tok(202)}, 9};
        p = Pair{};
        CHECK(once_each(200, 202) && p.a.get() == 0 && p.plain == 0);
        std::vector<Pair> v;
        for (int k = 0; k < 9; ++k) {
            Pair q{Tok(300 + 3 * k), {Tok(301 + 3 * k), Tok(302 + 3 * k)}, k};
            v.push_back(std::move(q));
        }
        CHECK(times(300) == 0 && times(326) == 0);
    }
    CHECK(once_each(300, 326));

    for (const auto& kv : g_released) CHECK(kv.second == 1);  // nothing released twice, anywhere above
    CHECK(g_released.count(0) == 0 && times(3) == 0);        // the empty value, and the one given up
    if (g_fail) return 1;
    std::printf("owned_check ok\n");
    return 0;
}
