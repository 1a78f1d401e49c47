// ray_key.hpp -- the 32-bit sort key of the coherent ray order (ceres_ray_order*), one function for
// the host (render_cpu.cpp) and the device (ray_order.hip), float and double.
//
//   bit  31      dead: the ray cannot reach the scene -- a NaN among its 8 numbers, a non-finite origin
//                or direction, a zero direction, !(tmin <= tmax), or an empty interval of the plain slab
//                test against the order box over [tmin, tmax].  A dead ray's key is 0x80000000: the dead
//                rays gather behind the live ones and fill whole wavefronts that end at once.
//   bits 30..28  the octant: the sign bits of d.x, d.y, d.z (bit 28 = x).  A wavefront of one octant
//                takes the octant-specialised box loop.
//   bits 27..7   the 21-bit Morton code (x lowest) of the cell of p = o + t0 d on a 128^3 grid over the
//                order box, t0 the start of the slab interval; p is clamped into the box, and an axis of
//                zero extent gives cell 0.
//   bits 6..0    0 (no direction detail): the sort skips them.
//
// The order box is the union of the boxes of the root's two children (pair 0 of the scene's sibling
// pairs), so every kind of scene -- float or double, device or host, refitted or rebuilt -- has it at
// hand without any state of its own.  It is usable when the root is not a leaf and its six numbers
// are finite with lo <= hi; else (a single-leaf scene, a soup with NaN triangles) no ray is dead by
// the box and every cell is 0.
//
// Only IEEE operations whose result does not depend on the compiler: - * / compare, select and a
// truncating conversion; every translation unit that includes this is built with -ffp-contract=off.
// A wrong or poor key can change a run time, never an answer.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define CERES_KEY_FN __host__ __device__ inline
#else
#define CERES_KEY_FN inline
#endif

namespace ceres {

constexpr uint32_t kRayKeyDead = 0x80000000u;
constexpr int kRayKeyBeginBit = 7, kRayKeyEndBit = 32;    // the bits the sort reads
constexpr int kRayKeyGrid = 128;

template <class S>
struct OrderBox {
    S lo[3], hi[3];
    bool ok;
};

template <class S>
CERES_KEY_FN bool key_finite(S x) { return x - x == S(0); }          // false for NaN and +-inf

// lb / rb: the two child boxes of pair 0 {xmin, xmax, ymin, ymax, zmin, zmax}.
template <class S>
CERES_KEY_FN OrderBox<S> order_box(const S* lb, const S* rb, uint32_t root_leaf_count) {
    OrderBox<S> b;
    b.ok = root_leaf_count == 0;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = lb[2 * a] < rb[2 * a] ? lb[2 * a] : rb[2 * a];
        b.hi[a] = lb[2 * a + 1] > rb[2 * a + 1] ? lb[2 * a + 1] : rb[2 * a + 1];
        b.ok = b.ok && key_finite(lb[2 * a]) && key_finite(rb[2 * a]) && key_finite(lb[2 * a + 1]) && key_finite(rb[2 * a + 1]) &&
               b.lo[a] <= b.hi[a];
    }
    return b;
}

CERES_KEY_FN uint32_t key_spread7(uint32_t c) {                       // bit i of c to bit 3 i
    uint32_t m = 0;
    for (int i = 0; i < 7; ++i) m |= ((c >> i) & 1u) << (3 * i);
    return m;
}

// sign: the sign bits of d (bit 0 = x), taken from the representation by the caller.
template <class S>
CERES_KEY_FN uint32_t ray_key(const S o[3], const S d[3], S tmin, S tmax, uint32_t sign, const OrderBox<S>& box) {
    bool dead = !(tmin <= tmax);                                      // a NaN bound too
    for (int a = 0; a < 3; ++a) dead = dead || !key_finite(o[a]) || !key_finite(d[a]);
    dead = dead || (d[0] == S(0) && d[1] == S(0) && d[2] == S(0));
    if (dead) return kRayKeyDead;
    uint32_t cell[3] = {0u, 0u, 0u};
    if (box.ok) {
        S t0 = tmin, t1 = tmax;
        bool empty = false;
        for (int a = 0; a < 3; ++a) {
            if (d[a] == S(0)) {
                empty = empty || !(box.lo[a] <= o[a] && o[a] <= box.hi[a]);
            } else {
                const S ta = (box.lo[a] - o[a]) / d[a], tb = (box.hi[a] - o[a]) / d[a];
                const S tn = ta < tb ? ta : tb, tf = ta < tb ? tb : ta;
                t0 = tn > t0 ? tn : t0;
                t1 = tf < t1 ? tf : t1;
            }
        }
        if (empty || !(t0 <= t1)) return kRayKeyDead;
        for (int a = 0; a < 3; ++a) {
            const S ext = box.hi[a] - box.lo[a];
            if (!(ext > S(0))) continue;                              // a flat axis: cell 0
            const S p = o[a] + t0 * d[a];
            const S f = (p - box.lo[a]) / ext * S(kRayKeyGrid);
            if (!(f >= S(0))) cell[a] = 0u;                           // below the box, or a NaN (inf * 0)
            else if (f >= S(kRayKeyGrid - 1)) cell[a] = uint32_t(kRayKeyGrid - 1);
            else cell[a] = uint32_t(f);                               // truncates; 0 <= f < 127
        }
    }
    const uint32_t morton = key_spread7(cell[0]) | (key_spread7(cell[1]) << 1) | (key_spread7(cell[2]) << 2);
    return ((sign & 7u) << 28) | (morton << 7);
}

}  // namespace ceres
