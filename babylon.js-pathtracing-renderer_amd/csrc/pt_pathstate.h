// pt_pathstate.h — CalculateRadiance's small per-path integers and flags (pt_program.h PState: diffuseCount,
// hitType, bounce, coat, specular, sampleLight) as one 32-bit word: the word of a pt_cont record (pt_trace.h
// contStore / contLoad) and the one register that carries them across a BVH walk (bounceStep), instead of
// three VGPRs and three lane masks. Plain C++ over plain numbers, no HIP (constexpr: host and device alike):
// tests/test_pathstate.py compiles it on its own.
//   bits 0-7 diffuseCount | 8-15 hitType (two's complement: -100 before the first hit) | 16-23 bounce |
//   24 coat | 25 specular | 26 sampleLight | 27-31 zero
#pragma once
#include <cstdint>

namespace pt {

struct PathBits {
    int diffuseCount, hitType, bounce;
    bool coat, specular, sampleLight;
};

constexpr uint32_t pathBitsPack(int diffuseCount, int hitType, int bounce, bool coat, bool specular, bool sampleLight)
{
    return ((uint32_t)diffuseCount & 0xffu) | (((uint32_t)hitType & 0xffu) << 8) | (((uint32_t)bounce & 0xffu) << 16) |
           (coat ? 1u << 24 : 0u) | (specular ? 1u << 25 : 0u) | (sampleLight ? 1u << 26 : 0u);
}
constexpr PathBits pathBitsUnpack(uint32_t bits)
{
    // hitType: the byte sign-extended without a conversion to a narrower signed type
    return PathBits{ (int)(bits & 0xffu), (int)(((bits >> 8) & 0xffu) ^ 0x80u) - 0x80, (int)((bits >> 16) & 0xffu),
                     ((bits >> 24) & 1u) != 0u, ((bits >> 25) & 1u) != 0u, ((bits >> 26) & 1u) != 0u };
}

} // namespace pt
