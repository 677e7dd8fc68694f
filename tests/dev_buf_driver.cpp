// Stand-alone driver of opt_amd/csrc/dev_buf.h for tests/test_dev_buf_cpu.py (built with -fsanitize=address,undefined, run as a child process): DevBuf over
// counting stand-ins for hipMalloc / hipFree.  Every allocation must be freed exactly once across reserve, reserve-larger, move-assign, release and scope exit.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
typedef void* hipStream_t;
static std::set<void*> live; static int nAlloc = 0, nFree = 0, nClear = 0;
static int fakeMalloc(void** p, size_t bytes) { *p = malloc(bytes); live.insert(*p); ++nAlloc; return 0; }
static int fakeFree(void* p) { if (live.erase(p) != 1) { printf("freed twice or never allocated\n"); exit(2); } free(p); ++nFree; return 0; }
static int fakeClear(void* p, int v, size_t bytes, hipStream_t) { for (size_t i = 0; i < bytes; ++i) ((char*)p)[i] = (char)v; ++nClear; return 0; }
#define hipMalloc fakeMalloc
#define hipFree fakeFree
#define hipMemsetAsync fakeClear
#define HIP_CHECK(call) do { if ((call) != 0) exit(3); } while (0)
#include "dev_buf.h"
#define REQUIRE(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    using optamd::DevBuf;
    {
        DevBuf<int> a, b;
        REQUIRE(a.p == nullptr && !a.reserve(0) && nAlloc == 0);
        REQUIRE(a.reserve(10) && a.cap == 10 && !a.reserve(10) && !a.reserve(3) && nAlloc == 1);      // grows only
        int* first = a;
        REQUIRE(a.reserve(11) && a.cap == 11 && nAlloc == 2 && nFree == 1 && !live.count(first));   // a larger request replaces the allocation
        REQUIRE(b.reserveZeroed(4, nullptr) && nClear == 1 && b.p[3] == 0 && !b.reserveZeroed(4, nullptr) && nClear == 1);
        int* kept = a;
        b = std::move(a);                                                                              // b's allocation goes, a's moves
        REQUIRE(b.p == kept && b.cap == 11 && a.p == nullptr && a.cap == 0 && nFree == 2 && live.size() == 1);
        b = std::move(b);
        REQUIRE(b.p == kept && live.size() == 1);
        DevBuf<int> c(std::move(b));
        REQUIRE(c.p == kept && b.p == nullptr);
        c.release(); c.release();
        REQUIRE(c.p == nullptr && c.cap == 0 && nFree == 3 && live.empty());
        REQUIRE(a.reserve(2) && b.reserve(5));                                                         // left to the destructors
    }
    REQUIRE(live.empty() && nAlloc == 5 && nFree == 5);
    printf("ok %d\n", nAlloc);
    return 0;
}
