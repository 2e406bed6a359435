// The layout of a caller-provided workspace: every plan builder (make_*_plan) reserves its slots from one WsLayout, in the
// order it names them, and reads the total off the end.  Plain C++, no HIP: usable from a host-only program.
#pragma once
#include <stddef.h>

namespace mmr {

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bump layout of 256-byte aligned slots.  take(bytes) returns the slot's offset; take(0) reserves nothing, which is how a
// plan spells "this slot is empty in this mode" (the offset it returns is then the next slot's and must not be used).
// A slot that has to exist whatever its size -- a one-value header, a sort's temporary storage whose size query may
// answer 0 -- asks for at least one byte.  After the last take, `off` is the workspace size.
struct WsLayout {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t at = off; off += align_up(bytes, 256); return at; }
};

}  // namespace mmr
