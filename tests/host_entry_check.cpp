// Stand-alone host check of csrc/host_entry.h, built with the host address and undefined-behaviour
// sanitizers by tests/test_workspace_layout_cpu.py. It drives Carver on a null base and on a malloc'd
// buffer of exactly the reported size, touches the first and last byte of every part, and drives
// require_pointers and require_workspace. No device call is made. Exit status 0 means every check held.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../bundlesdf_amd/csrc/host_entry.h"

static char g_error[256];
int nof::set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return code;
}

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

struct Part {
    char *p;
    size_t bytes;
};

// a layout with parts of 1-, 4-, 8- and 16-byte elements, as the match and pose-graph workspaces have
struct Layout : nof::Carver {
    std::vector<Part> parts;
    std::vector<size_t> starts;      // the running offset before each take
    Layout(void *base, size_t P, size_t L, size_t S) : Carver(base) {
        add<float>(P * L);
        add<float>(P * S);
        add<int32_t>(1);
        add<unsigned char>(P * L + 3);
        add<double>(6 * P);
        add<float4>(S);
        add<int64_t>(0);      // an empty part takes no room and stays in bounds
    }
    template <typename T> void add(size_t n) {
        starts.push_back(bytes);
        parts.push_back({reinterpret_cast<char *>(take<T>(n)), n * sizeof(T)});
    }
};

static int check_layout(size_t P, size_t L, size_t S) {
    const Layout sized(nullptr, P, L, S);
    const std::vector<size_t> &starts = sized.starts;
    CHECK(starts.size() == 7);
    for (const Part &q : sized.parts) CHECK(q.p == nullptr);
    CHECK(sized.bytes % 256 == 0 && sized.bytes >= 256);
    CHECK(starts[0] == 0);
    for (int i = 1; i < 7; ++i) CHECK(starts[i] % 256 == 0 && starts[i] >= starts[i - 1] + sized.parts[i - 1].bytes);
    char *buf = static_cast<char *>(malloc(sized.bytes));    // exactly the reported size: one byte past it is poisoned
    CHECK(buf);
    const Layout ws(buf, P, L, S);
    CHECK(ws.bytes == sized.bytes);
    for (size_t i = 0; i < ws.parts.size(); ++i) {
        const Part &q = ws.parts[i];
        CHECK(q.p == buf + starts[i]);
        CHECK(q.p >= buf && q.p + q.bytes <= buf + ws.bytes);
        if (q.bytes) q.p[0] = 1, q.p[q.bytes - 1] = 2;       // the sanitizer sees both ends of the part
        if (i + 1 < ws.parts.size()) CHECK(q.p + q.bytes <= ws.parts[i + 1].p);
    }
    free(buf);
    return 0;
}

int main() {
    if (check_layout(1, 1, 1) || check_layout(3, 100, 37) || check_layout(2, 70, 45) || check_layout(20, 2000, 64)) return 1;
    // a product past 2^32 is formed in size_t (null base: nothing is allocated)
    CHECK(nof::Carver(nullptr).take<float>((size_t)1 << 31) == nullptr);
    nof::Carver big(nullptr);
    big.take<double>((size_t)1 << 30);
    CHECK(big.bytes == (size_t)1 << 33);

    int a = 0, b = 0;
    CHECK(nof::require_pointers("fn", {}) == NOF_OK);
    CHECK(nof::require_pointers("fn", {{&a, "a"}, {&b, "b"}, {nullptr, "c", false}}) == NOF_OK);
    CHECK(nof::require_pointers("fn", {{nullptr, "a"}, {nullptr, "b"}}) == NOF_EINVAL && !strcmp(g_error, "fn: a is NULL"));
    CHECK(nof::require_pointers("fn", {{&a, "a"}, {nullptr, "b", false}, {nullptr, "c"}}) == NOF_EINVAL &&
          !strcmp(g_error, "fn: c is NULL"));
    CHECK(nof::require_workspace("fn", 512, 512) == NOF_OK);
    CHECK(nof::require_workspace("fn", 511, 512) == NOF_EINVAL &&
          !strcmp(g_error, "fn: workspace_bytes=511 is below the 512 bytes needed"));
    puts("host_entry_check: ok");
    return 0;
}
