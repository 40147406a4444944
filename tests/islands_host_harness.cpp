// Test-only: the component path's arithmetic (csrc/gs_device_math.h: gsm::NeighbourForEach over gsm::NeighbourRun, NeighbourBound, NeighbourRunEnd and
// NeighbourTest) compiled for the HOST and run serially the way the kernels of gs_neighbours.hip run it -- the list and its origin, the keys, a stable
// sort, the records, then per sorted position the edges to earlier positions into a union-find by sorted position, the component's smallest splat index
// and its size -- so that tests/test_islands_host.py can hold it to tests/islands_model.py integer for integer on a box without a GPU.  The union-find
// here is serial: what the lock-free one of cc_link does under interleavings is modelled in tests/test_islands_model.py.  Never part of the shipped library.
// A stand-alone program (its own main):  islands_host_harness <in> <out>
//   in : u32 n, f32 radius, n x 3 fp32 positions, n bytes (1 = alive)
//   out: n x u32 labels, then n x u32 sizes -- 0xFFFFFFFF and 0 for a splat that is not alive
// Without arguments it runs the same code over an input it makes itself and checks what needs no model: the form a sanitizer build runs.
// -DISLANDS_LABEL_IS_ROOT: a mutation for DESIGN.md section 4.18 -- the label is the index of the splat at the root position, not the minimum.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../unitygaussiansplatting_amd/csrc/gs_device_math.h"

static uint32_t find(std::vector<uint32_t>& parent, uint32_t x) {
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
}

static void run(const std::vector<float>& pos, const std::vector<uint8_t>& alive, float radius, std::vector<uint32_t>& labels, std::vector<uint32_t>& sizes) {
    const uint32_t n = (uint32_t)alive.size();
    labels.assign(n, 0u);
    sizes.assign(n, 0u);
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
    // link: union by sorted position, the larger root under the smaller
    std::vector<uint32_t> parent(m);
    for (uint32_t s = 0; s < m; ++s) parent[s] = s;
    const float r2 = radius * radius;
    for (uint32_t s = 0; s < m; ++s)
        gsm::NeighbourForEach(keys.data(), recs.data(), m, s, r2, [&](uint32_t j) {
            const uint32_t a = find(parent, s), b = find(parent, j);
            if (a != b) parent[a > b ? a : b] = a > b ? b : a;
        });
    // flatten, reduce, the outputs by splat index
    std::vector<uint32_t> root(m), minIdx(m, 0xFFFFFFFFu), size(m, 0u);
    for (uint32_t s = 0; s < m; ++s) root[s] = find(parent, s);
    for (uint32_t s = 0; s < m; ++s) { minIdx[root[s]] = std::min(minIdx[root[s]], recs[s].idx); ++size[root[s]]; }
    for (uint32_t s = 0; s < m; ++s) {
#ifdef ISLANDS_LABEL_IS_ROOT
        labels[recs[s].idx] = recs[root[s]].idx;
#else
        labels[recs[s].idx] = minIdx[root[s]];
#endif
        sizes[recs[s].idx] = size[root[s]];
    }
    for (uint32_t i = 0; i < n; ++i) {
        if (!alive[i]) { labels[i] = 0xFFFFFFFFu; sizes[i] = 0u; }
        else if (sizes[i] == 0u) { labels[i] = i; sizes[i] = 1u; }
    }
}

static int self_test() {
    // a 5 x 5 x 5 lattice of spacing 0.25 at radius 0.25 (one component through pairs at d2 == r2), a far identical pair, a NaN, a dead splat on the
    // lattice, and a lattice point deleted so that a corner hangs on nothing: index 0 is the corner (0, 0, 0), its three lattice neighbours are dead
    std::vector<float> pos;
    std::vector<uint8_t> alive;
    for (int z = 0; z < 5; ++z)
        for (int y = 0; y < 5; ++y)
            for (int x = 0; x < 5; ++x) { pos.push_back(0.25f * x); pos.push_back(0.25f * y); pos.push_back(0.25f * z); alive.push_back(1); }
    alive[1] = alive[5] = alive[25] = 0;
    const float far[2][3] = { { 3.0e9f, -2.0e9f, 1.0e9f }, { 3.0e9f, -2.0e9f, 1.0e9f } };
    for (const float* p : { far[0], far[1] }) { pos.insert(pos.end(), p, p + 3); alive.push_back(1); }
    pos.insert(pos.end(), { gsm::u2f(0x7fc00000u), 0.0f, 0.0f }); alive.push_back(1);
    pos.insert(pos.end(), { 0.5f, 0.5f, 0.5f }); alive.push_back(0);
    std::vector<uint32_t> l, s;
    run(pos, alive, 0.25f, l, s);
    bool ok = l[0] == 0u && s[0] == 1u && l[1] == 0xFFFFFFFFu && s[1] == 0u && l[2] == 2u && s[2] == 121u && l[124] == 2u && s[124] == 121u;
    ok = ok && l[125] == 125u && l[126] == 125u && s[125] == 2u && s[126] == 2u && l[127] == 127u && s[127] == 1u && l[128] == 0xFFFFFFFFu && s[128] == 0u;
    std::vector<uint32_t> l2, s2;
    run(pos, alive, 0.2f, l2, s2);                                 // below the spacing: every lattice point alone, the identical pair still one
    ok = ok && l2[62] == 62u && s2[62] == 1u && l2[126] == 125u && s2[125] == 2u;
    if (!ok) { fprintf(stderr, "components %u/%u %u/%u %u/%u %u/%u %u/%u\n", l[0], s[0], l[2], s[2], l[124], s[124], l[126], s[126], l[127], s[127]); return 1; }
    printf("islands_host_harness ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) return self_test();
    if (argc != 3) { fprintf(stderr, "usage: %s [<in> <out>]\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    uint32_t n = 0;
    float radius = 0.0f;
    bool ok = fread(&n, 4, 1, in) == 1 && fread(&radius, 4, 1, in) == 1;
    std::vector<float> pos(ok ? (size_t)n * 3 : 0);
    std::vector<uint8_t> alive(ok ? n : 0);
    ok = ok && (n == 0 || (fread(pos.data(), 4, pos.size(), in) == pos.size() && fread(alive.data(), 1, n, in) == n));
    fclose(in);
    if (!ok) { fprintf(stderr, "short input\n"); return 2; }
    std::vector<uint32_t> labels, sizes;
    run(pos, alive, radius, labels, sizes);
    FILE* f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    ok = n == 0 || (fwrite(labels.data(), 4, n, f) == n && fwrite(sizes.data(), 4, n, f) == n);
    if (fclose(f) != 0 || !ok) { fprintf(stderr, "short output\n"); return 2; }
    return 0;
}
