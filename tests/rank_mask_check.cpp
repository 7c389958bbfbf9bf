// Host check of bsk::rank_from_ballots (bspy_amd/csrc/bsk_rank.hpp): the mask arithmetic that follows the wave
// ballots of the row rotation's rank, against a brute-force count.  Stand-alone; built and run by
// tests/test_rank_mask.py.  TEST INFRASTRUCTURE.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../bspy_amd/csrc/bsk_rank.hpp"

static int failures = 0;

// One wave: cls[lane] < 2^NB, exec = the active lanes.  What the kernel does: a ballot per class bit (inactive lanes
// contribute 0), handed to every active lane; against: the number of active lanes below it in its half and class.
template <int NB>
static void check_wave(const char *what, const unsigned (&cls)[64], uint64_t exec)
{
    unsigned long long ballot[NB];
    for (int k = 0; k < NB; ++k) {
        ballot[k] = 0;
        for (int l = 0; l < 64; ++l)
            if (((exec >> l) & 1u) && ((cls[l] >> k) & 1u)) ballot[k] |= uint64_t(1) << l;
    }
    int count[2][1 << NB];
    memset(count, 0, sizeof(count));
    for (int l = 0; l < 64; ++l) {
        if (!((exec >> l) & 1u)) continue;                     // inactive lanes take no rank
        const int half = l >> 5;
        const int got = bsk::rank_from_ballots<NB>(ballot, exec, cls[l], l);
        int want = 0;
        for (int j = 32 * half; j < l; ++j)
            if (((exec >> j) & 1u) && cls[j] == cls[l]) ++want;
        if (got != want || got != count[half][cls[l]]) {
            if (failures < 20) printf("FAIL %s NB=%d lane %d class %u: rank %d, brute force %d\n", what, NB, l, cls[l], got, want);
            ++failures;
        }
        ++count[half][cls[l]];                                 // ranks of a class are 0, 1, 2, ... in lane order
    }
}

static const uint64_t EXECS[] = {
    ~uint64_t(0),                    // full wave
    uint64_t(1),                     // N = 1
    (uint64_t(1) << 33) - 1,         // low 33 lanes
    0xF0F0A5A5C3C3FF00ull,           // holes
    0x00000000FFFFFFFEull,           // lower half only, lane 0 off
    0xFFFFFFFF00000000ull,           // upper half only
    0x8000000080000001ull,
};

template <int NB>
static void check_all(const char *what, const unsigned (&cls)[64])
{
    for (uint64_t e : EXECS) check_wave<NB>(what, cls, e);
}

template <int NB>
static void run()
{
    constexpr unsigned NC = 1u << NB;
    unsigned cls[64];

    // all 64 lanes in one class: every class in turn
    for (unsigned c = 0; c < NC; ++c) {
        for (int l = 0; l < 64; ++l) cls[l] = c;
        check_all<NB>("one class", cls);
    }
    // classes with 0, 1, 4, 5 and 9 members per half (and the rest in one more class): 19 + 13 = 32
    {
        const int members[4] = {1, 4, 5, 9};
        for (unsigned shift = 0; shift < NC; ++shift) {
            for (int half = 0; half < 2; ++half) {
                int l = 32 * half;
                for (int g = 0; g < 4; ++g)
                    for (int i = 0; i < members[g]; ++i) cls[l++] = (shift + 1 + (unsigned)g) % NC;   // class `shift` stays empty
                while (l < 32 * half + 32) cls[l++] = (shift + 5) % NC;
            }
            check_all<NB>("0/1/4/5/9 members, blocks", cls);
            // the same members interleaved: lane order inside a class is not contiguous
            unsigned mixed[64];
            for (int l = 0; l < 64; ++l) mixed[l] = cls[(l & 32) + ((l * 7) & 31)];
            check_all<NB>("0/1/4/5/9 members, interleaved", mixed);
        }
    }
    // members of a class only in the upper half
    for (unsigned c = 0; c < NC; ++c) {
        for (int l = 0; l < 64; ++l) cls[l] = l < 32 ? (c + 1 + (unsigned)l % (NC - 1)) % NC : (l % 3 ? c : (c + 1) % NC);
        check_all<NB>("class in the upper half only", cls);
    }
    // consecutive lanes in consecutive classes
    for (int l = 0; l < 64; ++l) cls[l] = (unsigned)l % NC;
    check_all<NB>("sweep", cls);
    // random classes and random masks
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int rep = 0; rep < 2000; ++rep) {
        for (int l = 0; l < 64; ++l) cls[l] = (unsigned)(next() >> 40) % NC;
        check_wave<NB>("random", cls, next() | (rep & 1 ? next() : 0));
        check_wave<NB>("random", cls, ~uint64_t(0));
    }
}

int main()
{
    run<3>();   // order 4: 8 classes
    run<4>();   // order 2: 16 classes
    run<5>();   // 32 classes
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("rank mask ok\n");
    return 0;
}
