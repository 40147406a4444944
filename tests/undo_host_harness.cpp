// Test-only: the edit history's compaction arithmetic (csrc/gs_device_math.h: gsm::HistMaskedWord, HistBlockWords, HistBlockCount, HistRank) compiled for the
// HOST and run the way the kernels of gs_edit.hip run it -- hist_count per block, the scan, hist_gather per (block, thread), hist_swap per journal item -- so
// that tests/test_undo_model.py can hold it to tests/undo_model.py byte for byte on a box without a GPU.  Never part of the shipped library.
// A stand-alone program (its own main):  undo_host_harness <in> <out>
//   in : u32 n, u32 nWords, nWords selection words, then the state at the checkpoint (12 n, 16 n, 192 n bytes of pos / other / sh) and the state at the
//        undo (the same three)
//   out: u32 k, (n + 255) / 256 block counts, k indices, then the journal after the swap (12 k, 16 k, 192 k bytes) and the undo-time state after it
// Without arguments it runs the same code over an input it makes itself (513 splats, every third selected, the tail bits set) and checks what needs no
// model: the form a sanitizer build runs.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../unitygaussiansplatting_amd/csrc/gs_device_math.h"

static const size_t kStride[3] = { 12, 16, 192 };

struct Run {
    uint32_t n = 0, nWords = 0, k = 0;
    std::vector<uint32_t> sel, counts, idx;
    std::vector<uint8_t> then[3], now[3], journal[3];
};

// checkpoint in the state `then`, undo in the state `now`; false: a slot was out of range or taken twice
static bool emulate(Run& r) {
    const uint32_t n = r.n, nWords = r.nWords, blocks = (n + gsm::kHistBlock - 1u) / gsm::kHistBlock;
    // hist_count + the scan
    std::vector<uint32_t> base(blocks + 1u);
    r.counts.assign(blocks, 0u);
    for (uint32_t b = 0; b < blocks; ++b) {
        uint32_t m[8];
        gsm::HistBlockWords(r.sel.data(), nWords, n, b, m);
        r.counts[b] = gsm::HistBlockCount(m);
    }
    base[0] = 0u;
    for (uint32_t b = 0; b < blocks; ++b) base[b + 1u] = base[b] + r.counts[b];
    const uint32_t k = r.k = base[blocks];
    // hist_gather: every thread of every block, bits at indices >= n masked as the kernel masks them
    r.idx.assign(k, 0xFFFFFFFFu);
    for (int c = 0; c < 3; ++c) r.journal[c].assign((size_t)k * kStride[c], 0);
    for (uint32_t b = 0; b < blocks; ++b) {
        uint32_t m[8];
        gsm::HistBlockWords(r.sel.data(), nWords, n, b, m);
        for (uint32_t t = 0; t < gsm::kHistBlock; ++t) {
            if (!((m[t >> 5] >> (t & 31u)) & 1u)) continue;
            const uint32_t i = b * gsm::kHistBlock + t, slot = base[b] + gsm::HistRank(m, t);
            if (i >= n || slot >= k || r.idx[slot] != 0xFFFFFFFFu) { fprintf(stderr, "bad slot %u for splat %u\n", slot, i); return false; }
            r.idx[slot] = i;
            for (int c = 0; c < 3; ++c) memcpy(r.journal[c].data() + (size_t)slot * kStride[c], r.then[c].data() + (size_t)i * kStride[c], kStride[c]);
        }
    }
    // hist_swap: one journal item at a time
    for (uint32_t j = 0; j < k; ++j)
        for (int c = 0; c < 3; ++c) {
            uint8_t tmp[192];
            uint8_t* a = r.now[c].data() + (size_t)r.idx[j] * kStride[c];
            uint8_t* q = r.journal[c].data() + (size_t)j * kStride[c];
            memcpy(tmp, a, kStride[c]); memcpy(a, q, kStride[c]); memcpy(q, tmp, kStride[c]);
        }
    return true;
}

static int self_test() {
    Run r;
    r.n = 513; r.nWords = (r.n + 31u) / 32u;
    r.sel.assign(r.nWords, 0u);
    for (uint32_t i = 0; i < r.n; i += 3u) r.sel[i >> 5] |= 1u << (i & 31u);
    r.sel[r.nWords - 1u] |= ~0u << (r.n & 31u);                    // the tail bits
    uint32_t x = 12345u;
    for (int c = 0; c < 3; ++c) {
        r.then[c].resize((size_t)r.n * kStride[c]); r.now[c].resize(r.then[c].size());
        for (uint8_t& v : r.then[c]) { x = x * 1664525u + 1013904223u; v = (uint8_t)(x >> 24); }
        for (uint8_t& v : r.now[c]) { x = x * 1664525u + 1013904223u; v = (uint8_t)(x >> 24); }
    }
    const Run before = r;
    if (!emulate(r) || r.k != 171u) { fprintf(stderr, "k = %u\n", r.k); return 1; }
    for (uint32_t j = 0; j < r.k; ++j) {
        if (r.idx[j] != 3u * j) { fprintf(stderr, "idx[%u] = %u\n", j, r.idx[j]); return 1; }
        for (int c = 0; c < 3; ++c) {                              // the renderer holds the checkpoint's record, the entry the one it replaced
            if (memcmp(r.now[c].data() + (size_t)r.idx[j] * kStride[c], before.then[c].data() + (size_t)r.idx[j] * kStride[c], kStride[c]) != 0) return 1;
            if (memcmp(r.journal[c].data() + (size_t)j * kStride[c], before.now[c].data() + (size_t)r.idx[j] * kStride[c], kStride[c]) != 0) return 1;
        }
    }
    for (uint32_t i = 0; i < r.n; ++i)
        for (int c = 0; c < 3; ++c)
            if (i % 3u && memcmp(r.now[c].data() + (size_t)i * kStride[c], before.now[c].data() + (size_t)i * kStride[c], kStride[c]) != 0) return 1;
    printf("undo_host_harness ok\n");
    return 0;
}

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
static bool write_all(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc == 1) return self_test();
    if (argc != 3) { fprintf(stderr, "usage: %s [<in> <out>]\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    uint32_t head[2];
    if (!read_all(in, head, sizeof(head))) return 2;
    Run r;
    r.n = head[0]; r.nWords = head[1];
    r.sel.resize(r.nWords);
    bool ok = read_all(in, r.sel.data(), (size_t)r.nWords * 4);
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < 3; ++c) {
            std::vector<uint8_t>& b = (s == 0 ? r.then : r.now)[c];
            b.resize((size_t)r.n * kStride[c]);
            ok = ok && read_all(in, b.data(), b.size());
        }
    fclose(in);
    if (!ok) { fprintf(stderr, "short input\n"); return 2; }
    if (!emulate(r)) return 1;
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    ok = write_all(out, &r.k, 4) && write_all(out, r.counts.data(), r.counts.size() * 4) && write_all(out, r.idx.data(), (size_t)r.k * 4);
    for (int c = 0; c < 3; ++c) ok = ok && write_all(out, r.journal[c].data(), r.journal[c].size());
    for (int c = 0; c < 3; ++c) ok = ok && write_all(out, r.now[c].data(), r.now[c].size());
    if (fclose(out) != 0 || !ok) { fprintf(stderr, "short output\n"); return 2; }
    return 0;
}
