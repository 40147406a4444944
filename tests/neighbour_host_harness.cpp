// Test-only: the neighbour counts' arithmetic (csrc/gs_device_math.h: gsm::NeighbourFinite, NeighbourCellEdge, NeighbourKeyOf, NeighbourRun, NeighbourBound,
// NeighbourTest, NeighbourCount) compiled for the HOST and run serially the way the kernels of gs_neighbours.hip run it -- the list and its origin, the
// keys, a stable sort, the records, nine runs and the walk per sorted position -- so that tests/test_neighbour_host.py can hold it to
// tests/neighbour_model.py integer for integer on a box without a GPU.  Never part of the shipped library.
// A stand-alone program (its own main):  neighbour_host_harness <in> <out>
//   in : u32 n, f32 radius, u32 limit, n x 3 fp32 positions, n bytes (1 = alive)
//   out: n x u32 -- min(count, limit) of an alive splat, 0xFFFFFFFF of every other one
// Without arguments it runs the same code over an input it makes itself and checks what needs no model: the form a sanitizer build runs.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../unitygaussiansplatting_amd/csrc/gs_device_math.h"

static std::vector<uint32_t> run(const std::vector<float>& pos, const std::vector<uint8_t>& alive, float radius, uint32_t limit) {
    const uint32_t n = (uint32_t)alive.size();
    std::vector<uint32_t> out(n, 0u);
    // the list and its origin
    std::vector<uint32_t> list;
    const float inf = gsm::u2f(0x7f800000u);
    float origin[3] = { inf, inf, inf };
    for (uint32_t i = 0; i < n; ++i) {
        const gsm::V3 p = { pos[3 * i], pos[3 * i + 1], pos[3 * i + 2] };
        if (!alive[i] || !gsm::NeighbourFinite(p)) continue;
        list.push_back(i);
        origin[0] = fminf(origin[0], p.x); origin[1] = fminf(origin[1], p.y); origin[2] = fminf(origin[2], p.z);
    }
    const uint32_t m = (uint32_t)list.size();
    // keys, the stable sort, the records
    const double h = gsm::NeighbourCellEdge(radius);
    std::vector<unsigned long long> key(m);
    std::vector<uint32_t> rank(m);
    for (uint32_t j = 0; j < m; ++j) {
        const uint32_t i = list[j];
        key[j] = gsm::NeighbourKeyOf({ pos[3 * i], pos[3 * i + 1], pos[3 * i + 2] }, origin, h);
        rank[j] = j;
    }
    std::stable_sort(rank.begin(), rank.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    std::vector<gsm::NeighbourRec> recs(m);
    std::vector<unsigned long long> keys(m);
    for (uint32_t s = 0; s < m; ++s) {
        const uint32_t i = list[rank[s]];
        recs[s] = { pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], i };
        keys[s] = key[rank[s]];
    }
    // the walk
    const float r2 = radius * radius;
    for (uint32_t s = 0; s < m; ++s) {
        uint32_t tests = 0u;
        out[recs[s].idx] = gsm::NeighbourCount(keys.data(), recs.data(), m, s, r2, limit, tests);
    }
    for (uint32_t i = 0; i < n; ++i)
        if (!alive[i]) out[i] = 0xFFFFFFFFu;
    return out;
}

static int self_test() {
    // a 7 x 7 x 7 lattice of spacing 0.25 at radius 0.25 (an inner point has six neighbours at d2 == r2), a far pair, a NaN and a dead splat
    std::vector<float> pos;
    std::vector<uint8_t> alive;
    for (int z = 0; z < 7; ++z)
        for (int y = 0; y < 7; ++y)
            for (int x = 0; x < 7; ++x) { pos.push_back(0.25f * x); pos.push_back(0.25f * y); pos.push_back(0.25f * z); alive.push_back(1); }
    const float far[2][3] = { { 3.0e9f, -2.0e9f, 1.0e9f }, { 3.0e9f, -2.0e9f, 1.0e9f } };
    for (const float* p : { far[0], far[1] }) { pos.insert(pos.end(), p, p + 3); alive.push_back(1); }
    pos.insert(pos.end(), { gsm::u2f(0x7fc00000u), 0.0f, 0.0f }); alive.push_back(1);
    pos.insert(pos.end(), { 0.75f, 0.75f, 0.75f }); alive.push_back(0);                    // on the centre point, dead
    const std::vector<uint32_t> c = run(pos, alive, 0.25f, 65535u);
    const uint32_t centre = 3u + 7u * (3u + 7u * 3u);
    bool ok = c[centre] == 6u && c[0] == 3u && c[343] == 1u && c[344] == 1u && c[345] == 0u && c[346] == 0xFFFFFFFFu;
    const std::vector<uint32_t> c2 = run(pos, alive, 0.25f, 2u);
    ok = ok && c2[centre] == 2u && c2[343] == 1u && c2[345] == 0u;
    const std::vector<uint32_t> c0 = run(pos, alive, 0.25f, 0u);
    ok = ok && c0[centre] == 0u;
    if (!ok) { fprintf(stderr, "counts %u %u %u %u %u %u / %u\n", c[centre], c[0], c[343], c[344], c[345], c[346], c2[centre]); return 1; }
    printf("neighbour_host_harness ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) return self_test();
    if (argc != 3) { fprintf(stderr, "usage: %s [<in> <out>]\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    uint32_t n = 0, limit = 0;
    float radius = 0.0f;
    bool ok = fread(&n, 4, 1, in) == 1 && fread(&radius, 4, 1, in) == 1 && fread(&limit, 4, 1, in) == 1;
    std::vector<float> pos(ok ? (size_t)n * 3 : 0);
    std::vector<uint8_t> alive(ok ? n : 0);
    ok = ok && (n == 0 || (fread(pos.data(), 4, pos.size(), in) == pos.size() && fread(alive.data(), 1, n, in) == n));
    fclose(in);
    if (!ok) { fprintf(stderr, "short input\n"); return 2; }
    const std::vector<uint32_t> out = run(pos, alive, radius, limit);
    FILE* f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    ok = n == 0 || fwrite(out.data(), 4, n, f) == n;
    if (fclose(f) != 0 || !ok) { fprintf(stderr, "short output\n"); return 2; }
    return 0;
}
