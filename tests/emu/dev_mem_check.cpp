// TEST INFRASTRUCTURE: moshpp_amd/csrc/dev_mem.h on its own, against tests/emu/fakehip (whose hipMalloc counts calls and live
// allocations and fails the n-th on request).  Prints one line per case: "<case> <numbers...>"; tests/test_dev_mem.py holds them.
#include "dev_mem.h"

#include <cstdio>
#include <cstring>

// what the stand-in header expects of the fiber scheduler (hip_emu_runtime.cpp), which this program does not link
namespace hipemu { long malloc_calls = 0, live_allocs = 0, fail_malloc_in = 0; void register_dynamic_lds(double*, size_t) {} }
static int g_fail_code = 0;
extern "C" int moshii_internal_fail(int code, const char*) { g_fail_code = code; return code; }

static long live() { return hipemu::live_allocs; }

// one host-buffer call as the entries make it: two inputs, a null optional input, two outputs, a null optional output
static int staged_call(uint32_t flags, const double* a, const int* b, double* out, int* out2, long* live_inside) {
    Staging st(flags, nullptr);
    const double* d_a = st.in(a, 4);
    const int* d_b = st.in(b, 3);
    const float* d_none = st.in((const float*)nullptr, 5);
    double* d_out = st.out(out, 4);
    int* d_out2 = st.out(out2, 3);
    float* d_opt = st.out((float*)nullptr, 7);
    *live_inside = live();
    if (!st.ok()) return 1;
    if (d_none || d_opt) return 2;
    if (st.device() && (d_a != a || d_b != b || d_out != out || d_out2 != out2)) return 3;
    if (!st.device() && (d_a == a || d_b == b || d_out == out || d_out2 == out2)) return 4;
    for (int i = 0; i < 4; ++i) d_out[i] = 2.0 * d_a[i];     // the "kernel"
    for (int i = 0; i < 3; ++i) d_out2[i] = d_b[i] + 1;
    return st.finish() == hipSuccess ? 0 : 5;
}

int main() {
    {   // alloc / upload / zeros, then the destructor
        const long before = live();
        {
            DevArena a;
            const int src[3] = {7, 8, 9};
            int* p = a.upload(src, 3);
            double* z = a.zeros<double>(5, nullptr);
            char* e = a.alloc<char>(0);          // never null on success
            int* none = a.upload(src, 0);        // nothing to upload: null, no allocation, still ok
            double sum = 0.0;
            for (int i = 0; i < 5; ++i) sum += z[i];
            printf("arena %d %zu %ld %d %d %d %d\n", (int)a.ok(), a.count(), live() - before, p[0] + p[1] + p[2], (int)(sum == 0.0), (int)(e != nullptr),
                   (int)(none == nullptr));
        }
        printf("arena_gone %ld\n", live() - before);
    }
    {   // clear, move construction, move assignment over live contents
        const long before = live();
        DevArena a, b;
        a.alloc<int>(4); a.alloc<int>(4);
        b.alloc<int>(4);
        const long l0 = live() - before;         // 3
        DevArena c(std::move(a));                // c owns a's two, a is empty
        const long l1 = live() - before;         // 3
        const size_t ca = a.count(), cc = c.count();
        b = std::move(c);                        // b's one is freed, b owns the two
        const long l2 = live() - before;         // 2
        const size_t cb = b.count(), cc2 = c.count();
        b.clear();
        const long l3 = live() - before;         // 0
        b.alloc<int>(1);                         // usable after clear
        printf("moves %ld %ld %zu %zu %ld %zu %zu %ld %zu\n", l0, l1, ca, cc, l2, cb, cc2, l3, b.count());
    }
    {   // a failed allocation is sticky: null from then on, nothing further is tried, what was made is still owned and freed
        const long before = live();
        long calls_after_failure;
        {
            DevArena a;
            a.alloc<int>(2);
            hipemu::fail_malloc_in = 1;
            int* bad = a.alloc<int>(2);
            const long calls = hipemu::malloc_calls;
            int* later = a.alloc<int>(2);
            calls_after_failure = hipemu::malloc_calls - calls;
            printf("sticky %d %d %d %zu %ld %ld\n", (int)a.ok(), (int)(bad == nullptr), (int)(later == nullptr), a.count(), live() - before, calls_after_failure);
            a.clear();                           // clear() also forgets the failure
            printf("sticky_cleared %d %ld\n", (int)a.ok(), live() - before);
        }
    }
    {   // a staged call in both modes; then the n-th allocation of the host-mode call fails, every n
        const double a[4] = {1, 2, 3, 4};
        const int b[3] = {10, 20, 30};
        double out[4] = {0, 0, 0, 0}, guard = -1.0;
        int out2[3] = {0, 0, 0};
        long inside = 0;
        const long before = live(), calls0 = hipemu::malloc_calls;
        int rc = staged_call(MOSHII_BUFFERS_HOST, a, b, out, out2, &inside);
        const long n = hipemu::malloc_calls - calls0;
        printf("staged_host %d %ld %ld %ld %g %g %d %g\n", rc, n, inside - before, live() - before, out[0], out[3], out2[2], guard);
        double dout[4] = {0, 0, 0, 0};
        int dout2[3] = {0, 0, 0};
        const long calls1 = hipemu::malloc_calls;
        rc = staged_call(MOSHII_BUFFERS_DEVICE, a, b, dout, dout2, &inside);
        printf("staged_device %d %ld %ld %g %d\n", rc, hipemu::malloc_calls - calls1, inside - before, dout[3], dout2[0]);
        for (long nth = 1; nth <= n; ++nth) {
            double o[4] = {-5, -5, -5, -5};
            int o2[3] = {-5, -5, -5};
            hipemu::fail_malloc_in = nth;
            rc = staged_call(MOSHII_BUFFERS_HOST, a, b, o, o2, &inside);
            hipemu::fail_malloc_in = 0;
            printf("staged_fail_%ld %d %ld %ld %g %d\n", nth, rc, inside - before, live() - before, o[0], o2[0]);   // outputs untouched
        }
    }
    {   // finish() copies back exactly what was recorded, once
        Staging st(MOSHII_BUFFERS_HOST, nullptr);
        double host[3] = {0, 0, 0};
        double* d = st.out(host, 2);             // two of the three elements
        d[0] = 1.5; d[1] = 2.5;
        st.finish();
        d[0] = 9.0;
        st.finish();                             // nothing is recorded any more
        printf("finish %g %g %g\n", host[0], host[1], host[2]);
    }
    {   // Scratch: grows, keeps, frees
        const long before = live();
        {
            Scratch s;
            const int r0 = s.reserve(100);
            const size_t cap0 = s.cap;
            const int r1 = s.reserve(1000);      // within the 64 KiB it starts with
            const long l1 = live() - before;
            const int r2 = s.reserve(100000);
            const size_t cap2 = s.cap;
            hipemu::fail_malloc_in = 1;
            const int r3 = s.reserve(1000000);
            hipemu::fail_malloc_in = 0;
            printf("scratch %d %zu %d %ld %d %zu %d %d %zu %ld\n", r0, cap0, r1, l1, r2, cap2, r3, g_fail_code, s.cap, live() - before);
        }
        printf("scratch_gone %ld\n", live() - before);
    }
    printf("end %ld\n", live());
    return 0;
}
