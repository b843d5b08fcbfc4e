// Host build of the PRODUCT header gfxexp_amd/csrc/emitter_cull.h for tests/test_emitter_cull.py: the builder and the predicate
// the kernels call (lights.hip k_emitter_records, restir.hip candidate_live), over arrays.
#include <stddef.h>
#include "../../gfxexp_amd/csrc/emitter_cull.h"

extern "C" {

// n records: m9[9 n] normal-matrix rows, nA / pA / pB / pC [3 n], flat / finiteEmittance [n] -> entries[4 n]
void cull_build_many(uint32_t n, const float* m9, const float* nA, const uint8_t* flat, const float* pA, const float* pB, const float* pC,
                     const uint8_t* finiteEmittance, uint32_t* entries) {
    for (uint32_t i = 0; i < n; ++i) {
        const gfx::EmitterCull e = gfx::cull_build(m9 + 9 * i, nA + 3 * i, flat[i] != 0, pA + 3 * i, pB + 3 * i, pC + 3 * i, finiteEmittance[i] != 0);
        entries[4 * i] = e.octN; entries[4 * i + 1] = gfx::cull_bits(e.hLo); entries[4 * i + 2] = e.cxy; entries[4 * i + 3] = e.czr;
    }
}

// every shading point (p, n, vz)[P] against every entry [K] -> skip[P K]
void cull_predicate_grid(uint32_t P, uint32_t K, const uint32_t* entries, const float* p, const float* n, const float* vz, uint8_t* skip) {
    for (uint32_t i = 0; i < P; ++i)
        for (uint32_t k = 0; k < K; ++k) {
            gfx::EmitterCull e;
            e.octN = entries[4 * k]; e.hLo = gfx::cull_float(entries[4 * k + 1]); e.cxy = entries[4 * k + 2]; e.czr = entries[4 * k + 3];
            skip[static_cast<size_t>(i) * K + k] = gfx::cull_proves_zero(e, p[3 * i], p[3 * i + 1], p[3 * i + 2], n[3 * i], n[3 * i + 1], n[3 * i + 2], vz[i]) ? 1 : 0;
        }
}

// the decoded entry: N[3], hLo, c[3], r
void cull_decode(const uint32_t* entry, float* out8) {
    gfx::cull_oct_decode(entry[0], out8[0], out8[1], out8[2]);
    out8[3] = gfx::cull_float(entry[1]);
    out8[4] = gfx::cull_half_to_float(entry[2] & 0xFFFFu); out8[5] = gfx::cull_half_to_float(entry[2] >> 16);
    out8[6] = gfx::cull_half_to_float(entry[3] & 0xFFFFu); out8[7] = gfx::cull_half_to_float(entry[3] >> 16);
}

// fp16 helpers: every finite pattern converts back and forth, rounding up never rounds down
int cull_half_selftest() {
    for (uint32_t h = 0x0400u; h < 0x7C00u; ++h) {
        const float f = gfx::cull_half_to_float(h);
        bool ok = true;
        if (gfx::cull_float_to_half_trunc(f, ok) != h || !ok) return 1;
        if (gfx::cull_float_to_half_up(f) != h) return 2;
        const float above = gfx::cull_float(gfx::cull_bits(f) + 1u);
        if (gfx::cull_float_to_half_up(above) != h + 1u) return 3;
        if (gfx::cull_float_to_half_trunc(above, ok) != h) return 4;
        if (gfx::cull_half_to_float(h | 0x8000u) != -f) return 5;
    }
    bool ok = true;
    gfx::cull_float_to_half_trunc(1e6f, ok);
    if (ok) return 6;
    if (gfx::cull_float_to_half_up(1e6f) != gfx::kCullHalfInf || gfx::cull_float_to_half_up(gfx::cull_float(0x7FC00000u)) != gfx::kCullHalfInf) return 7;
    if (gfx::cull_float_to_half_up(0.0f) != 0x0400u) return 8;
    return 0;
}

}
