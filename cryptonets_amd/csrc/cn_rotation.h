// The hops of a RotateRows, decided here and nowhere else: the Galois element of a step count and the key switches a rotation by `steps` takes with the keys at hand
// (Evaluator::rotate_internal of SEAL 3.2: the step's own key if present, otherwise the terms of its non-adjacent form).  Queue-time checks, the planner of
// cn_rotate_rows_many and the executing loop all read the same plan.  Host-only and free of HIP: a plain C++ compiler builds it (tests/cpp/rotation_plan.cpp).
#pragma once
#include "../../include/cnhip.h"

// 3^steps mod 2N for a rotation to the left by `steps` slots of a row (N/2 slots; negative: to the right), 2N - 1 - the column swap - for 0, 0 for |steps| >= N/2
inline uint64_t cn_elt_of_step(uint64_t n, int steps) {
    const uint64_t m = 2 * n;
    if (steps == 0) return m - 1;
    const uint64_t pos = steps < 0 ? 0 - (uint64_t)(int64_t)steps : (uint64_t)steps;
    if (pos >= n / 2) return 0;
    uint64_t e = 1, b = 3;
    for (uint64_t s = steps < 0 ? n / 2 - pos : pos; s; s >>= 1) { if (s & 1) e = (e * b) & (m - 1); b = (b * b) & (m - 1); }
    return e;
}

static const uint32_t CN_ROT_MAX_HOPS = 32;      // (the non-adjacent form of a 32-bit count has at most 17 terms)
struct CnRotPlan {
    int rc = 0; const char *msg = nullptr;        // the refusal: CN_ERR_ARG / CN_ERR_NOKEY and its text
    uint32_t hops = 0; uint64_t elt[CN_ROT_MAX_HOPS];    // Galois elements in execution order (no heap: a per-ciphertext caller plans thousands of rotations per image)
    CnRotPlan &refuse(int code, const char *text) { rc = code; msg = text; hops = 0; return *this; }
};
// have_key(elt): does the context hold the Galois key of this element?  The direct key wins; otherwise the terms of the non-adjacent form from low order first, each a
// power of two that needs its own key (its own form is the single term itself: no further split).  A term of N/2 is a whole turn of the row and is skipped.
// (One hop is always the step's own key: N/2 - 2^i has the element of -2^i.)
template <class HaveKey> inline CnRotPlan cn_rotation_plan(uint32_t n, int steps, HaveKey have_key) {
    CnRotPlan p;
    if (steps == 0) return p;
    const uint64_t own = cn_elt_of_step(n, steps);
    if (!own) return p.refuse(CN_ERR_ARG, "step count too large");
    if (have_key(own)) { p.elt[p.hops++] = own; return p; }
    int v = steps < 0 ? -steps : steps;           // (< N/2)
    for (int i = 0; v; i++) {
        const int zi = (v & 1) ? 2 - (v & 3) : 0;
        v = (v - zi) >> 1;
        if (!zi || (1u << i) == n / 2) continue;
        const uint64_t e = cn_elt_of_step(n, (steps < 0 ? -zi : zi) * (1 << i));
        if (!e) return p.refuse(CN_ERR_ARG, "step count too large");
        if (!have_key(e)) return p.refuse(CN_ERR_NOKEY, "Galois key not present");     // (a single-term form is the step itself, whose key is missing)
        p.elt[p.hops++] = e;
    }
    return p;
}
