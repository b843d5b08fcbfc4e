// tfdm_instance.hip.h -- displaced objects as instances of a scene: the arithmetic shared by k_scene_instances (tfdm_set.hip),
// the host side of the instance set and the tests (tests/scene_trace_host.cpp).  The reference does this work inside optixTrace
// on an instance AS that holds triangle GASes and custom-primitive GASes (tfdm/tfdm_main.cpp:2620-2640): the world ray goes to
// the instance's object space, the custom-primitive program runs there, and the closest-hit program brings the object-space
// normal back through the instance's normal matrix (tfdm_shared.h:570-577).
//
// Under the math contract of tfdm_core.hip.h: plain C++17, no contraction, selects for min and max; hipcc compiles it for the
// device and g++ for the host to the same bits.
//
// The merge rule of a scene query.  The closest hit wins; on equal distance a plain hit beats a displaced one and a lower
// instance index beats a higher one.  tfdm::trace_ray accepts only t < tmax, so walking the instances in index order and
// handing the best distance so far in as tmax (the plain hit first) is this rule: scene_instance() below does one step of it.
#pragma once
#include "tfdm_core.hip.h"
#include "tfdm_build.h"

namespace gfx {
namespace tfdm {

constexpr uint32_t kMaxInstances = 1024u;
constexpr uint32_t kScenePlain = 0x80000000u;           // GFX_SCENE_PLAIN

// One displaced instance, 12 x 16 bytes.  Matrices are row-major 3 x 4 as gfx_instance_set_transform takes them; the normal
// matrix is the transposed upper-left 3 x 3 of worldToObj.  The pointers are the member object's device buffers (host arrays
// in the tests): a record is valid for the object's generation it was made from.
struct alignas(16) InstanceRecord {
    float objToWorld[12];
    float worldToObj[12];    // the inverse in double of the float entries above, rounded to float
    float boxLo[3];          // the padded world box (make_instance)
    uint32_t userId;
    float boxHi[3];
    uint32_t pad0;
    const Node* nodes;
    const TriRecord* records;
    const float* heights;
    const F2* pyramid;
    Params params;
};
static_assert(sizeof(InstanceRecord) == 192, "InstanceRecord is 12 x 16 bytes");
static_assert(sizeof(void*) == 8, "InstanceRecord holds four 8-byte pointers");

// closest-hit record of a scene query (gfx_scene_hit)
struct SceneHit { float dist, bcB, bcC; uint32_t index; V3 normal; uint32_t where; };

GFX_TFDM_FN SceneHit scene_miss(float tmax) {
    SceneHit h;
    h.dist = tmax; h.bcB = 0.0f; h.bcC = 0.0f; h.index = kInvalid; h.normal = v3(0.0f, 0.0f, 0.0f); h.where = kInvalid;
    return h;
}
// what the plain phase found (a gfx_hit): triIndex kInvalid is a miss, whatever its distance says
GFX_TFDM_FN SceneHit scene_start(float tmax, float dist, float bcB, float bcC, uint32_t triIndex) {
    SceneHit h = scene_miss(tmax);
    if (triIndex != kInvalid) { h.dist = dist; h.bcB = bcB; h.bcC = bcC; h.index = triIndex; h.where = kScenePlain; }
    return h;
}

// World ray -> object ray: the origin as a point, the direction as a vector.  The direction is NOT renormalised, so a distance
// along the object ray is the world ray's parameter (optixGetObjectRayDirection).
GFX_TFDM_FN void to_object_ray(const InstanceRecord& r, V3 org, V3 dir, V3& objOrg, V3& objDir) {
    objOrg = mul3(r.worldToObj, 4, org) + v3(r.worldToObj[3], r.worldToObj[7], r.worldToObj[11]);
    objDir = mul3(r.worldToObj, 4, dir);
}

// The normal matrix (the transposed 3 x 3 of worldToObj) times an object-space normal, normalised.  It keeps the side: for a
// mirrored instance too, dot(world normal, world direction) has the sign of dot(object normal, object direction).
GFX_TFDM_FN V3 normal_to_world(const InstanceRecord& r, V3 n) {
    const float* m = r.worldToObj;
    return normalize(v3(m[0] * n.x + m[4] * n.y + m[8] * n.z, m[1] * n.x + m[5] * n.y + m[9] * n.z, m[2] * n.x + m[6] * n.y + m[10] * n.z));
}

// Slab test of the world ray against the instance's padded world box, inside [tmin, best]: false only where the object-space
// traversal would not get past its root box either (the pad of make_instance covers the rounding of to_object_ray).
GFX_TFDM_FN bool world_box_hit(const InstanceRecord& r, V3 org, V3 inv, float tmin, float best) {
    Box b;
    b.lo = v3(r.boxLo[0], r.boxLo[1], r.boxLo[2]);
    b.hi = v3(r.boxHi[0], r.boxHi[1], r.boxHi[2]);
    float t0, t1;
    V3 nearT, farT;
    return box_hit(b, org, inv, tmin, best, t0, t1, nearT, farT);
}

// One step of the merge rule: instance `index` against the world ray, accepted only where closer than `best`.  kAny: returns at
// the first hit and leaves `best` alone.  `stack` is emptied first (an any-hit return leaves entries behind).
template <bool kAny, bool kWithBilinear, class Stack>
GFX_TFDM_FN bool scene_instance_local(const InstanceRecord& r, uint32_t index, V3 org, V3 dir, float tmin, Stack& stack, SceneHit& best, TraceStats& ts) {
    V3 objOrg, objDir;
    to_object_ray(r, org, dir, objOrg, objDir);
    Map map;
    map.heights = r.heights; map.pyramid = r.pyramid;
    TraceHit h;
    stack.sp = 0;
    if (!trace_ray_local<kAny, kWithBilinear>(r.nodes, r.records, map, r.params, objOrg, objDir, tmin, best.dist, stack, h, ts)) return false;
    if (!kAny) {
        best.dist = h.t; best.bcB = h.bcB; best.bcC = h.bcC; best.index = h.prim;
        best.normal = normal_to_world(r, h.normal);
        best.where = (index << 1) | h.frontFace;
    }
    return true;
}
// ... with the instantiation chosen by the instance's mode (the host; k_scene_instances names its own)
template <bool kAny, class Stack>
GFX_TFDM_FN bool scene_instance(const InstanceRecord& r, uint32_t index, V3 org, V3 dir, float tmin, Stack& stack, SceneHit& best, TraceStats& ts) {
    if (r.params.local == kBilinear) return scene_instance_local<kAny, true>(r, index, org, dir, tmin, stack, best, ts);
    return scene_instance_local<kAny, false>(r, index, org, dir, tmin, stack, best, ts);
}

// ---------------------------------------------------------------- host: a record from a transform and an object
inline float round_down(double d) { const float f = static_cast<float>(d); return static_cast<double>(f) > d ? next_down(f) : f; }
inline float round_up(double d) { const float f = static_cast<float>(d); return static_cast<double>(f) < d ? next_up(f) : f; }

// Fills `out` (whole: padding zeroed) or returns a message.  The inverse is computed in double from the float entries and
// rounded to float.  The world box is the float64 image of the eight corners of the object's root box, rounded outward, then
// padded on every side by 2^-16 x (its largest |coordinate| + its largest extent): to_object_ray costs a few ulp (about 2^-22
// of those magnitudes), the pad is a safety factor of 64 over that, not a measurement.  A root box that is not finite (an
// affine bound that gave up) makes the world box everything.
inline const char* make_instance(const float objToWorld[12], const Node& root, const Node* nodes, const TriRecord* records, const float* heights,
                                 const F2* pyramid, const Params& params, uint32_t userId, InstanceRecord& out) {
    std::memset(&out, 0, sizeof(out));
    for (int i = 0; i < 12; ++i) if (!std::isfinite(objToWorld[i])) return "an entry of the instance transform is not finite";
    double m[9], mi[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) m[3 * r + c] = objToWorld[4 * r + c];
    // Singular for a float matrix: a determinant below 2^-20 of the product of its row lengths, that is rows coplanar to within
    // 2^-20 whatever their scales.  A singular matrix rounded to float has about 2^-24 there, not zero; and where a float entry's
    // own 2^-24 moves the inverse by 2^-4 of itself, an object ray made with it means nothing.
    double scale = 1.0;
    for (int r = 0; r < 3; ++r) scale *= std::sqrt(m[3 * r] * m[3 * r] + m[3 * r + 1] * m[3 * r + 1] + m[3 * r + 2] * m[3 * r + 2]);
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) + m[1] * (m[5] * m[6] - m[3] * m[8]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (!(std::fabs(det) > scale * (1.0 / 1048576.0)) || !invert3(m, mi)) return "the instance transform is singular";
    float w[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) w[4 * r + c] = static_cast<float>(mi[3 * r + c]);
        w[4 * r + 3] = static_cast<float>(-(mi[3 * r] * objToWorld[3] + mi[3 * r + 1] * objToWorld[7] + mi[3 * r + 2] * objToWorld[11]));
    }
    for (int i = 0; i < 12; ++i) if (!std::isfinite(w[i])) return "the instance transform is singular (its inverse does not fit a float)";
    for (int i = 0; i < 12; ++i) { out.objToWorld[i] = objToWorld[i]; out.worldToObj[i] = w[i]; }
    out.userId = userId;
    out.nodes = nodes; out.records = records; out.heights = heights; out.pyramid = pyramid;
    out.params = params;
    bool finite = true;
    for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(root.lo[k]) && std::isfinite(root.hi[k]);
    if (!finite) {
        for (int k = 0; k < 3; ++k) { out.boxLo[k] = -inf(); out.boxHi[k] = inf(); }
        return nullptr;
    }
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int corner = 0; corner < 8; ++corner) {
        const double p[3] = { (corner & 1) ? root.hi[0] : root.lo[0], (corner & 2) ? root.hi[1] : root.lo[1], (corner & 4) ? root.hi[2] : root.lo[2] };
        for (int r = 0; r < 3; ++r) {
            const double v = (static_cast<double>(objToWorld[4 * r]) * p[0] + static_cast<double>(objToWorld[4 * r + 1]) * p[1]) +
                             (static_cast<double>(objToWorld[4 * r + 2]) * p[2] + static_cast<double>(objToWorld[4 * r + 3]));
            lo[r] = std::min(lo[r], v); hi[r] = std::max(hi[r], v);
        }
    }
    double maxAbs = 0.0, maxExt = 0.0;
    float flo[3], fhi[3];
    for (int k = 0; k < 3; ++k) {
        flo[k] = round_down(lo[k]); fhi[k] = round_up(hi[k]);
        maxAbs = std::max(maxAbs, std::max(std::fabs(static_cast<double>(flo[k])), std::fabs(static_cast<double>(fhi[k]))));
        maxExt = std::max(maxExt, static_cast<double>(fhi[k]) - static_cast<double>(flo[k]));
    }
    const double pad = (maxAbs + maxExt) * (1.0 / 65536.0);
    for (int k = 0; k < 3; ++k) { out.boxLo[k] = round_down(static_cast<double>(flo[k]) - pad); out.boxHi[k] = round_up(static_cast<double>(fhi[k]) + pad); }
    return nullptr;
}

// ---------------------------------------------------------------- host: the motion of an instance between two commits
// curToPrev = prev * inverse(cur) (tfdm/tfdm_main.cpp:2476): takes a world point of the instance now to where that point of the
// instance was (row-major 3 x 4).  Computed in double from the float entries and rounded to float once, as make_instance makes
// worldToObj; `cur` is a transform make_instance accepted.  prev equal to cur bit for bit gives the exact identity, not the
// rounded product: an instance that did not move has the bytes of one that never moved.  Returns a message where `prev` is not
// finite or the result does not fit a float.
inline const char* make_cur_to_prev(const float prev[12], const float cur[12], float out[12]) {
    static const float ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    if (std::memcmp(prev, cur, sizeof(float) * 12) == 0) { std::memcpy(out, ident, sizeof(ident)); return nullptr; }
    for (int i = 0; i < 12; ++i) if (!std::isfinite(prev[i])) return "an entry of the instance's previous transform is not finite";
    double m[9], mi[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) m[3 * r + c] = cur[4 * r + c];
    if (!invert3(m, mi)) return "the instance transform is singular";
    for (int r = 0; r < 3; ++r) {
        double row[3];
        for (int c = 0; c < 3; ++c)
            row[c] = (static_cast<double>(prev[4 * r]) * mi[c] + static_cast<double>(prev[4 * r + 1]) * mi[3 + c]) + static_cast<double>(prev[4 * r + 2]) * mi[6 + c];
        const double t = static_cast<double>(prev[4 * r + 3]) -
                         ((row[0] * static_cast<double>(cur[3]) + row[1] * static_cast<double>(cur[7])) + row[2] * static_cast<double>(cur[11]));
        for (int c = 0; c < 3; ++c) out[4 * r + c] = static_cast<float>(row[c]);
        out[4 * r + 3] = static_cast<float>(t);
    }
    for (int i = 0; i < 12; ++i) if (!std::isfinite(out[i])) return "the motion of the instance does not fit a float";
    return nullptr;
}

} // namespace tfdm
} // namespace gfx
