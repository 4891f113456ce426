// air_check -- the host twin of the air interface (include/nfc_amd.h: nfc_host_air_render; csrc/air.hip.h) over frames made
// here: reader and tag frames of every length from a lone REQA to 256 bytes, ragged streams with an empty one among them, all four kinds,
// two rates, with and without noise -- rendered into heap blocks of EXACTLY the size the sizing call reports, so that a sample written
// past a stream's end, or a bit read past a frame's bytes, is a sanitizer finding.  A stand-alone host program: the way to run the
// twin's host code under a sanitizer.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined tools/air_check/main.cpp \
//         usrp_nfc_amd/csrc/nfc_air.hip -o air_check && ./air_check
// It touches no GPU.  Exit status 0: every rendering fits its block to the byte; a stream rendered alone under its stream seed has the
// bytes it has among others; a buffer one sample short is refused and left untouched;
// every argument error is NFC_ERR_ARG.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nfc_amd.h"

static std::string g_error;
namespace nfc {
void note_call_error(const char *text) { g_error = text; }   // (the library's is in nfc_amd.hip, behind nfc_last_error)
}

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

struct Streams {
    std::vector<nfc_air_frame> frames;
    std::vector<uint32_t> frame_off{0}, byte_base{0};
    std::vector<uint8_t> air, par;
    void frame(uint8_t type, uint16_t n_bits, uint32_t idle, uint32_t &seed) {
        nfc_air_frame f;
        memset(&f, 0, sizeof f);
        f.type = type, f.n_bits = n_bits, f.idle_before = idle, f.byte_off = (uint32_t)air.size() - byte_base.back();
        const uint32_t nb = n_bits == 0 ? 0 : n_bits <= 8 ? 1 : n_bits / 9;
        for (uint32_t i = 0; i < nb; i++) air.push_back((uint8_t)(lcg(seed) >> 24)), par.push_back((uint8_t)(lcg(seed) >> 31));
        frames.push_back(f);
    }
    void end_stream() { frame_off.push_back((uint32_t)frames.size()), byte_base.push_back((uint32_t)air.size()); }
    size_t K() const { return frame_off.size() - 1; }
};

static nfc_air_config config(uint32_t kind, double rate, float sigma, uint32_t align, uint32_t tail) {
    nfc_air_config c;
    memset(&c, 0, sizeof c);
    c.rate_msps = rate, c.carrier_i = 0.4776682f, c.carrier_q = 0.1477601f, c.depth = 0.08f, c.sigma = sigma;
    c.full_scale = kind == NFC_IN_IQ_I16 ? 32767.f : 127.f, c.out_kind = kind, c.seed = 0x14443A, c.tail = tail, c.align_samples = align;
    return c;
}
static size_t bps(uint32_t kind) { return kind == NFC_IN_IQ_F32 ? 8 : kind == NFC_IN_IQ_I16 ? 4 : 2; }

// the rendering in a block of exactly the reported size; empty on failure
static std::vector<uint8_t> render(const Streams &s, const nfc_air_config &c, std::vector<uint64_t> &first, std::vector<uint32_t> &n) {
    const size_t K = s.K();
    first.assign(K, 0), n.assign(K, 0);
    if (nfc_host_air_render(&c, s.frames.data(), s.frame_off.data(), s.air.data(), s.par.data(), s.byte_base.data(), K, nullptr, 0, first.data(), n.data()) != NFC_OK)
        return {};
    const size_t need = (size_t)(first[K - 1] + n[K - 1]);
    uint8_t *block = (uint8_t *)malloc(need * bps(c.out_kind) + 1);   // (malloc, not a vector: the red zone starts at the last byte)
    std::vector<uint8_t> out;
    if (nfc_host_air_render(&c, s.frames.data(), s.frame_off.data(), s.air.data(), s.par.data(), s.byte_base.data(), K, block, need, first.data(), n.data()) == NFC_OK)
        out.assign(block, block + need * bps(c.out_kind));
    if (need) {   // one sample short: refused, nothing written
        memset(block, 0x5A, need * bps(c.out_kind));
        const int rc = nfc_host_air_render(&c, s.frames.data(), s.frame_off.data(), s.air.data(), s.par.data(), s.byte_base.data(), K, block, need - 1, first.data(), n.data());
        for (size_t i = 0; i < need * bps(c.out_kind); i++)
            if (rc != NFC_ERR_ARG || block[i] != 0x5A) out.clear();
        if (g_error.find("cap_samples") == std::string::npos) out.clear();
    }
    free(block);
    return out;
}

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "air_check: line %d: %s\n", __LINE__, #cond); \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main() {
    uint32_t seed = 14443;
    Streams s;
    // stream 0: frames of both types and many lengths; 1: empty; 2: a lone REQA; 3: the longest frames; 4: frames without bits and without idle
    const uint16_t lens[] = {7, 18, 45, 1, 8, 9, 81, 162, 36};
    for (int i = 0; i < 9; i++) s.frame((uint8_t)(i & 1), lens[i], i ? 300 : 3000, seed);
    s.end_stream();
    s.end_stream();
    s.frame(1, 7, 3000, seed);
    s.end_stream();
    s.frame(1, 2304, 0, seed), s.frame(0, 2304, 1, seed);
    s.end_stream();
    s.frame(0, 0, 5, seed), s.frame(1, 0, 0, seed), s.frame(0, 27, 0, seed), s.frame(1, 27, 0, seed);
    s.end_stream();
    const uint32_t kinds[4] = {NFC_IN_IQ_F32, NFC_IN_IQ_I16, NFC_IN_IQ_I8, NFC_IN_IQ_U8};
    const uint64_t seeds[5] = {50, 40, 30, 20, 10};
    int renders = 0;
    for (uint32_t kind : kinds)
        for (double rate : {2.0, 13.56})
            for (float sigma : {0.f, 0.002f})
                for (uint32_t align : {1u, 64u})
                    for (uint32_t tail : {0u, 700u}) {
                        nfc_air_config c = config(kind, rate, sigma, align, tail);
                        c.stream_seeds = seeds;
                        std::vector<uint64_t> first, f1;
                        std::vector<uint32_t> n, n1;
                        const std::vector<uint8_t> all = render(s, c, first, n);
                        CHECK(!all.empty());
                        CHECK(n[1] == tail && first[0] == 0);
                        for (size_t k = 0; k < s.K(); k++) CHECK(first[k] % align == 0);
                        // stream 3 alone, under its seed: the bytes it has among the others
                        Streams one;
                        one.frames.assign(s.frames.begin() + s.frame_off[3], s.frames.begin() + s.frame_off[4]);
                        one.air.assign(s.air.begin() + s.byte_base[3], s.air.begin() + s.byte_base[4]);
                        one.par.assign(s.par.begin() + s.byte_base[3], s.par.begin() + s.byte_base[4]);
                        one.end_stream();
                        c.stream_seeds = seeds + 3;
                        const std::vector<uint8_t> alone = render(one, c, f1, n1);
                        CHECK(n1[0] == n[3] && alone.size() >= (size_t)n[3] * bps(kind));
                        CHECK(memcmp(alone.data(), all.data() + first[3] * bps(kind), (size_t)n[3] * bps(kind)) == 0);
                        renders++;
                    }
    // argument errors
    std::vector<uint64_t> first(s.K());
    std::vector<uint32_t> n(s.K());
    auto call = [&](const nfc_air_config &c, const Streams &t, size_t K) {
        return nfc_host_air_render(&c, t.frames.data(), t.frame_off.data(), t.air.data(), t.par.data(), t.byte_base.data(), K, nullptr, 0, first.data(), n.data());
    };
    nfc_air_config c = config(NFC_IN_IQ_F32, 2.0, 0.002f, 8, 400);
    CHECK(call(c, s, s.K()) == NFC_OK);
    c.out_kind = NFC_IN_ENV_F32;
    CHECK(call(c, s, s.K()) == NFC_ERR_ARG && g_error.find("out_kind") != std::string::npos);
    c = config(NFC_IN_IQ_F32, 2.0, 0.002f, 24, 400);
    CHECK(call(c, s, s.K()) == NFC_ERR_ARG && g_error.find("align_samples") != std::string::npos);
    c = config(NFC_IN_IQ_F32, 2.0, 0.002f, 8, 400);
    c.reserved[3] = 1;
    CHECK(call(c, s, s.K()) == NFC_ERR_ARG && g_error.find("reserved") != std::string::npos);
    c.reserved[3] = 0;
    CHECK(call(c, s, 65537) == NFC_ERR_ARG && g_error.find("K exceeds") != std::string::npos);
    Streams bad = s;
    bad.frames[3].n_bits = 10;
    CHECK(call(c, bad, s.K()) == NFC_ERR_ARG && g_error.find("frames[3].n_bits") != std::string::npos);
    bad = s;
    bad.frames[8].n_bits = 9 * 200;   // the stream's last frame: its bytes would come from the next streams' parts
    CHECK(call(c, bad, s.K()) == NFC_ERR_ARG && g_error.find("frames[8].byte_off") != std::string::npos);
    bad = s;
    bad.frames[0].reserved = 7;
    CHECK(call(c, bad, s.K()) == NFC_ERR_ARG && g_error.find("reserved") != std::string::npos);
    printf("air_check ok: %d renderings in blocks of the exact size, %zu streams, %zu frames\n", renders, s.K(), s.frames.size());
    return 0;
}
