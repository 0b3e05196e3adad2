// Host helpers of the C entry points: the workspace carver and the shared refusals. Host only.
#pragma once
#include <initializer_list>

#include "nof_device.h"

namespace nof {

// Walks a workspace part by part, each part starting on a 256-byte boundary. A file states a layout once:
// a struct of typed pointers derived from Carver whose constructor (base, shape) takes the parts in order.
// The *_workspace_bytes export builds it on a null base and reads `bytes`, the entry point builds it on the
// caller's buffer and uses the pointers. A null base yields null parts: no arithmetic is done on it.
struct Carver {
    char *base;
    size_t bytes = 0;               // offset of the next part; after the last take, the workspace's size
    explicit Carver(void *b) : base(static_cast<char *>(b)) {}
    template <typename T> T *take(size_t count) {
        T *p = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
        bytes += align256(count * sizeof(T));
        return p;
    }
};

// NOF_OK, or the refusal of the first needed null pointer in list order
struct NamedPointer { const void *p; const char *name; bool need = true; };
inline int require_pointers(const char *fn, std::initializer_list<NamedPointer> ptrs) {
    for (const NamedPointer &a : ptrs)
        if (a.need && !a.p) return set_error(NOF_EINVAL, "%s: %s is NULL", fn, a.name);
    return NOF_OK;
}
// NOF_OK, or the refusal of a buffer of `have` bytes, held in the descriptor field `what`, where `need` are used
inline int require_workspace(const char *fn, size_t have, size_t need, const char *what = "workspace_bytes") {
    return have >= need ? NOF_OK : set_error(NOF_EINVAL, "%s: %s=%zu is below the %zu bytes needed", fn, what, have, need);
}

}  // namespace nof
