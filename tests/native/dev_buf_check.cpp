// dev_buf_check.cpp -- DevBuf (csrc/dev_buf.h) against a counting stand-in for the caching allocator: every block that
// is handed out goes back exactly once, whatever way the owner ends.  Stand-alone host program, no HIP:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined dev_buf_check.cpp && ./a.out
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <utility>
#include <vector>
#include "../../zksnake_amd/csrc/dev_buf.h"

static std::vector<void*> g_out, g_back;   // every pointer handed out / returned, in order
static int g_fail_in = 0;                  // 1: the next allocation fails, 2: the one after it, ...; 0: none
static const int FAIL_STATUS = 7;

namespace zkmi {
int dev_alloc_cached(void** p, size_t bytes) {
    if (g_fail_in > 0 && --g_fail_in == 0) {
        *p = reinterpret_cast<void*>(0x1);   // an owner must not keep what a failing call left behind
        return FAIL_STATUS;
    }
    *p = malloc(bytes ? bytes : 1);
    g_out.push_back(*p);
    return 0;
}
void dev_free_cached(void* p) {
    if (!p) return;
    g_back.push_back(p);
}
}  // namespace zkmi

using zkmi::mem::DevBuf;

static int g_errors = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("  FAILED line %d: %s\n", __LINE__, #cond); ++g_errors; } \
    } while (0)

// handed out == returned as sets, nothing returned twice, nothing returned that was never handed out; then start afresh
static void settle(const char* what) {
    const int before = g_errors;
    CHECK(g_out.size() == g_back.size());
    for (size_t i = 0; i < g_back.size(); ++i) {
        size_t handed = 0, returned = 0;
        for (void* q : g_out) handed += q == g_back[i];
        for (void* q : g_back) returned += q == g_back[i];
        CHECK(handed == 1 && returned == 1);
    }
    for (void* q : g_out) free(q);   // only now, so that malloc cannot hand the same address out twice within a case
    g_out.clear();
    g_back.clear();
    printf("%s: %s\n", what, g_errors == before ? "ok" : "FAILED");
}

static int three_buffers(bool fail_late) {
    DevBuf a, b, c;
    if (int rc = a.alloc(16)) return rc;
    if (int rc = b.alloc(32)) return rc;
    if (int rc = c.alloc(64)) return rc;
    if (fail_late) return -1;   // a failing call after all three exist
    return 0;
}

int main() {
    {
        {
            DevBuf b;
            CHECK(!b && b.as() == nullptr);
            CHECK(b.alloc(64) == 0);
            CHECK(b && b.as<char>() == g_out[0]);
            b.as()[15] = 1;   // 64 bytes of uint32_t
            CHECK(g_back.empty());
        }
        CHECK(g_back.size() == 1);
        settle("scope end");
    }
    {
        DevBuf b;
        CHECK(b.alloc(8) == 0);
        void* first = b.as<void>();
        CHECK(b.alloc(24) == 0);
        CHECK(g_back.size() == 1 && g_back[0] == first);   // the old block went back before the new one came
        CHECK(b.as<void>() == g_out[1] && g_out[1] != first);
        b.reset();
        settle("alloc on a holder");
    }
    {
        DevBuf b;
        g_fail_in = 1;
        CHECK(b.alloc(8) == FAIL_STATUS);
        CHECK(!b && b.as() == nullptr);
        CHECK(b.alloc(8) == 0);
        g_fail_in = 1;
        CHECK(b.alloc(8) == FAIL_STATUS);   // the held block still goes back first
        CHECK(!b && g_back.size() == 1);
        b.reset();
        settle("failing alloc");
    }
    {
        {
            DevBuf a;
            CHECK(a.alloc(8) == 0);
            void* p = a.as<void>();
            DevBuf b(std::move(a));
            CHECK(!a && b.as<void>() == p && g_back.empty());
            DevBuf c;
            CHECK(c.alloc(8) == 0);
            void* held = c.as<void>();
            c = std::move(b);
            CHECK(!b && c.as<void>() == p);
            CHECK(g_back.size() == 1 && g_back[0] == held);   // the target gave up what it held; the source frees nothing
            DevBuf& same = c;
            c = std::move(same);
            CHECK(c.as<void>() == p && g_back.size() == 1);
        }
        CHECK(g_back.size() == 2);
        settle("move");
    }
    {
        DevBuf b;
        CHECK(b.alloc(8) == 0);
        b.reset();
        b.reset();
        CHECK(!b && g_back.size() == 1);
        settle("reset twice");
    }
    {
        auto one = std::make_shared<DevBuf>();
        CHECK(one->alloc(128) == 0);
        std::shared_ptr<DevBuf> two = one;
        one.reset();
        CHECK(g_back.empty() && *two);
        two.reset();
        CHECK(g_back.size() == 1);
        settle("shared_ptr with two holders");
    }
    {
        CHECK(three_buffers(true) == -1);
        CHECK(g_out.size() == 3 && g_back.size() == 3);
        g_fail_in = 3;
        CHECK(three_buffers(false) == FAIL_STATUS);   // the third allocation fails: the first two go back
        CHECK(g_out.size() == 5 && g_back.size() == 5);
        g_fail_in = 1;
        CHECK(three_buffers(false) == FAIL_STATUS);   // none exists yet
        CHECK(g_out.size() == 5 && g_back.size() == 5);
        CHECK(three_buffers(false) == 0);
        CHECK(g_out.size() == 8 && g_back.size() == 8);
        settle("early return with three buffers");
    }
    if (g_errors) printf("dev_buf_check: %d FAILED\n", g_errors);
    else printf("dev_buf_check: all ok\n");
    return g_errors ? 1 : 0;
}
