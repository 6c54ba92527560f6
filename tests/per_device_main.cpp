// Stand-alone check of m3dssd_amd/csrc/per_device.h (host compiler only; tests/test_per_device_host.py builds it plain, with
// -fsanitize=thread and with -fsanitize=address,undefined, and runs each binary).  Exit status 0 and "PER_DEVICE_OK" = all held.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "per_device.h"

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

int main()
{
    // 1. 8 threads x 1000 gets over 4 ordinals: every init hands out a DIFFERENT number (a ticket), so a caller that saw anything
    //    but the slot's one value -- a second init's result, a half-published slot -- shows up as a mismatch
    {
        static PerDevice<int> pd;
        std::atomic<int> tickets{0}, mismatches{0};
        int seen[8][4];
        std::vector<std::thread> th;
        for (int t = 0; t < 8; ++t)
            th.emplace_back([&, t]() {
                for (int d = 0; d < 4; ++d) seen[t][d] = -1;
                for (int i = 0; i < 1000; ++i) {
                    const int d = (i + t) % 4;
                    const std::optional<int> v = pd.get(d, [&]() { return std::optional<int>(1000 * (d + 1) + tickets.fetch_add(1)); });
                    if (!v || *v / 1000 != d + 1) { mismatches.fetch_add(1); continue; }
                    if (seen[t][d] < 0) seen[t][d] = *v;
                    if (seen[t][d] != *v) mismatches.fetch_add(1);
                }
            });
        for (auto &x : th) x.join();
        CHECK(mismatches.load() == 0);
        CHECK(tickets.load() == 4);                                  // one successful init per ordinal
        for (int t = 1; t < 8; ++t)
            for (int d = 0; d < 4; ++d) CHECK(seen[t][d] == seen[0][d]);
    }
    // 2. a failing init is handed back, not cached, and tried again; the first success sticks
    {
        PerDevice<int> pd;
        int calls = 0;
        auto flaky = [&]() -> std::optional<int> { return ++calls < 3 ? std::nullopt : std::optional<int>(40 + calls); };
        CHECK(!pd.get(5, flaky) && calls == 1);
        CHECK(!pd.get(5, flaky) && calls == 2);
        CHECK(pd.get(5, flaky) == std::optional<int>(43) && calls == 3);
        CHECK(pd.get(5, flaky) == std::optional<int>(43) && calls == 3);
        CHECK(!pd.get(6, [&]() -> std::optional<int> { return std::nullopt; }));      // another ordinal is still empty
    }
    // 3. ordinals outside [0, 64) are computed on every call
    {
        PerDevice<int> pd;
        int calls = 0;
        auto count = [&]() { return std::optional<int>(++calls); };
        for (int i = 1; i <= 3; ++i) CHECK(pd.get(-1, count) == std::optional<int>(i));
        for (int i = 4; i <= 6; ++i) CHECK(pd.get(M3D_MAX_DEVICES, count) == std::optional<int>(i));
        CHECK(calls == 6);
        CHECK(pd.get(M3D_MAX_DEVICES - 1, count) == std::optional<int>(7) && pd.get(M3D_MAX_DEVICES - 1, count) == std::optional<int>(7));
        CHECK(pd.get(0, count) == std::optional<int>(8) && pd.get(0, count) == std::optional<int>(8) && calls == 8);
    }
    // 4. two objects do not share slots
    {
        PerDevice<int> a, b;
        CHECK(a.get(2, []() { return std::optional<int>(11); }) == std::optional<int>(11));
        CHECK(b.get(2, []() { return std::optional<int>(22); }) == std::optional<int>(22));
        CHECK(a.get(2, []() { return std::optional<int>(33); }) == std::optional<int>(11));
        PerDevice<const float *> p;                                                        // (the zero page's type)
        static const float z = 0.f;
        CHECK(p.get(2, []() { return std::optional<const float *>(&z); }).value_or(nullptr) == &z);
    }
    if (g_fail) return 1;
    std::puts("PER_DEVICE_OK");
    return 0;
}
