// ctx_commands_check -- nfc_host_commands_segmented (include/nfc_amd.h; csrc/ctx_commands.hip.h: the cuts, the speculative walks and the
// resolve in the text the kernels run) against nfc_host_commands_keyed, the sequential twin, on the same raw frames: the records, data,
// enc and the state afterwards must be equal byte for byte, in ascending, reversed and shuffled segment order.
//   1. the routes tests/test_ctx_commands_host.py renders (write_routes: a session ended by an encrypted HALT; the Classic prefix cut off
//      in mid-session before three Ultralight transactions; the cur_key one transaction leaves to the next), read from the file named on
//      the command line -- without one this part is skipped and says so;
//   2. 10 000 random frame lists: protocol-shaped frames (REQA, WUPA, ATQA, anticollision, SELECT, SAK, AUTHA / AUTHB, nonces, HALT)
//      and noise in random order, from random start states with and without a session, with and without a sector key table, whole and
//      in two batches.
// Every buffer has exactly the capacity the frames need, so that a write past a frame's slot is a write past an allocation.
// A stand-alone host program: the way to run this host code under a sanitizer.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/ctx_commands_check/main.cpp \
//         usrp_nfc_amd/csrc/nfc_ctx_commands.hip usrp_nfc_amd/csrc/nfc_commands.hip -o ctx_commands_check && ./ctx_commands_check [routes.bin]
// It touches no GPU.  Exit status 0: everything equal.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nfc_amd.h"

struct Input {
    nfc_fsm_state st;
    nfc_fsm_key_table table;
    bool keyed;
    std::vector<nfc_raw_frame> frames;
    std::vector<uint8_t> bytes[2], par[2];
};
struct Result {
    std::vector<nfc_frame> fr;
    std::vector<uint8_t> data;
    std::vector<uint16_t> enc;
    nfc_fsm_state st;
    bool operator==(const Result &o) const {
        return fr.size() == o.fr.size() && (fr.empty() || memcmp(fr.data(), o.fr.data(), fr.size() * sizeof(nfc_frame)) == 0) && data == o.data &&
               enc == o.enc && memcmp(&st, &o.st, sizeof st) == 0;
    }
};
static int fail(const char *what, long where = -1) {
    printf("ctx_commands_check: %s (%ld)\n", what, where);
    return 1;
}
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static uint32_t below(uint32_t n) { return rnd() % n; }

static size_t slots_of(const Input &in, size_t a, size_t b) {
    size_t n = 0;
    for (size_t i = a; i < b; i++) n += (in.frames[i].flags & NFC_RAW_CUT) ? 0 : in.frames[i].n_bytes;
    return n;
}
// frames [a, b) from `st`: order 0 the sequential twin, 1 / 2 / 3 the segmented one ascending / reversed / shuffled
static bool run(const Input &in, size_t a, size_t b, const nfc_fsm_state &st, int order, Result &r, nfc_ctx_command_counters *cn) {
    const size_t n = b - a, cap = slots_of(in, a, b);
    r.fr.assign(n, nfc_frame()), r.data.assign(cap, 0xEE), r.enc.assign(cap, 0xEEEE);
    r.st = st;
    size_t used = 0;
    const nfc_fsm_key_table *tab = in.keyed ? &in.table : nullptr;
    const nfc_raw_frame *fr = n ? in.frames.data() + a : nullptr;
    int rc;
    if (order == 0) {
        rc = nfc_host_commands_keyed(&r.st, tab, fr, n, in.bytes[0].data(), in.par[0].data(), in.bytes[1].data(), in.par[1].data(), r.fr.data(),
                                     r.data.data(), r.enc.data(), cap, &used);
    } else {
        std::vector<uint32_t> ord(n + 1);
        for (size_t i = 0; i <= n; i++) ord[i] = (uint32_t)(order == 2 ? n - i : i);
        if (order == 3)
            for (size_t i = n; i > 0; i--) std::swap(ord[i], ord[below((uint32_t)i + 1)]);
        rc = nfc_host_commands_segmented(&r.st, tab, fr, n, in.bytes[0].data(), in.par[0].data(), in.bytes[1].data(), in.par[1].data(), r.fr.data(),
                                         r.data.data(), r.enc.data(), cap, &used, order == 1 ? nullptr : ord.data(), order == 1 ? 0 : ord.size(), cn);
    }
    return rc == NFC_OK && used == cap;
}
// whole, and in two batches cut at `cut` with the state carried: every order equals the sequential twin
static int check(const Input &in, size_t cut, nfc_ctx_command_counters *total) {
    const size_t n = in.frames.size();
    for (int pass = 0; pass < 2; pass++) {
        nfc_fsm_state st = in.st;
        const size_t parts[3] = {0, pass ? cut : n, n};
        for (int p = 0; p < (pass ? 2 : 1); p++) {
            Result want, got;
            if (!run(in, parts[p], parts[p + 1], st, 0, want, nullptr)) return fail("nfc_host_commands_keyed refused the list");
            for (int order = 1; order <= 3; order++) {
                nfc_ctx_command_counters cn;
                if (!run(in, parts[p], parts[p + 1], st, order, got, &cn)) return fail("nfc_host_commands_segmented refused the list", order);
                if (!(got == want)) return fail("the segmented twin differs from the sequential one", order);
                if (order == 1 && pass == 0 && total)
                    total->n_segments += cn.n_segments, total->n_rerun_segments += cn.n_rerun_segments, total->n_rerun_frames += cn.n_rerun_frames,
                        total->n_keydep_segments += cn.n_keydep_segments;
            }
            st = want.st;
        }
    }
    return 0;
}

// ---- random lists ----
static void put_frame(Input &in, int type, const std::vector<uint8_t> &data, bool good_parity, bool with_crc) {
    std::vector<uint8_t> d = data;
    if (with_crc) {
        uint8_t c[2];
        nfc_crc_a(d.data(), d.size(), c);
        d.push_back(c[0]), d.push_back(c[1]);
    }
    nfc_raw_frame r;
    memset(&r, 0, sizeof r);
    r.idx = in.frames.size(), r.type = type, r.byte_off = (uint32_t)in.bytes[type].size(), r.n_bytes = (uint32_t)d.size(), r.n_bits = 9 * r.n_bytes;
    bool ok = !d.empty();
    for (size_t i = 0; i < d.size(); i++) {
        uint8_t p = (uint8_t)(1 - (__builtin_popcount(d[i]) & 1));
        if (!good_parity && below(3) == 0) p ^= 1, ok = false;
        in.bytes[type].push_back(d[i]), in.par[type].push_back(p);
    }
    if (ok) {
        r.flags |= NFC_RAW_PARITY_OK;
        uint8_t c[2];
        if (d.size() >= 2 && nfc_crc_a(d.data(), d.size() - 2, c) == NFC_OK && c[0] == d[d.size() - 2] && c[1] == d[d.size() - 1]) r.flags |= NFC_RAW_CRC_A_OK;
    }
    if (below(40) == 0) r.flags |= below(2) ? NFC_FRAME_EXTRA_ERROR : NFC_FRAME_MANY_MORE_ERROR;
    if (below(60) == 0) r.flags = NFC_RAW_CUT, r.n_bytes = 0;   // (its bytes stay in the arrays: nobody reads them)
    in.frames.push_back(r);
}
static std::vector<uint8_t> noise(size_t n) {
    std::vector<uint8_t> d(n);
    for (auto &b : d) b = (uint8_t)rnd();
    return d;
}
static Input random_input() {
    Input in;
    nfc_fsm_state_init(&in.st);
    nfc_fsm_key_table_init(&in.table);
    in.keyed = below(3) == 0;
    if (in.keyed)
        for (int t = 0; t < 2; t++)
            for (int s = 0; s < NFC_KEY_SECTORS; s++)
                if (below(4) == 0) {
                    in.table.present[t][s] = 1;
                    for (int i = 0; i < 6; i++) in.table.key[t][s][i] = (uint8_t)rnd();
                }
    for (int i = 0; i < 6; i++) in.st.key_a[i] = (uint8_t)rnd(), in.st.key_b[i] = (uint8_t)rnd();
    if (below(2)) {   // a machine somewhere in a stream
        in.st.cur_cmd = (int32_t)below((uint32_t)nfc_command_count());
        in.st.tag_type = (int32_t)below(5) - 1;
        in.st.encrypted = (int32_t)below(3);
        in.st.cur_key = below(2) ? (int32_t)below(2) : (int32_t)(2 + below(80));
        in.st.cipher = ((uint64_t)rnd() << 16) ^ rnd();
        in.st.cipher &= (1ull << 48) - 1;
        for (int i = 0; i < 4; i++) in.st.ar[i] = (uint8_t)rnd(), in.st.at[i] = (uint8_t)rnd();
        in.st.uid_len = below(3) == 0 ? 7 : 4 * below(2);
        for (uint32_t i = 0; i < in.st.uid_len; i++) in.st.uid[i] = (uint8_t)rnd();
        in.st.flags = below(4);
    }
    const uint8_t uid[4] = {(uint8_t)rnd(), (uint8_t)rnd(), (uint8_t)rnd(), (uint8_t)rnd()};
    const uint8_t bcc = uid[0] ^ uid[1] ^ uid[2] ^ uid[3];
    const size_t n = below(48);
    uint32_t step = 0;
    while (in.frames.size() < n) {
        const uint32_t what = below(8) ? step++ % 11 : below(14);   // mostly in protocol order, sometimes anything
        const bool good = below(12) != 0;
        switch (what) {
        case 0: put_frame(in, 1, {(uint8_t)(below(4) ? 0x26 : 0x52)}, good, false); break;
        case 1: put_frame(in, 0, {(uint8_t)(below(2) ? 0x04 : 0x44), 0x00}, good, false); break;
        case 2: put_frame(in, 1, {0x93, 0x20}, good, false); break;
        case 3: put_frame(in, 0, {uid[0], uid[1], uid[2], uid[3], bcc}, good, false); break;
        case 4: put_frame(in, 1, {0x93, 0x70, uid[0], uid[1], uid[2], uid[3], bcc}, good, true); break;
        case 5: put_frame(in, 0, {(uint8_t)(below(2) ? 0x08 : 0x04)}, good, true); break;
        case 6:
            if (below(2)) put_frame(in, 1, {(uint8_t)(0x60 + below(2)), (uint8_t)rnd()}, good, true);
            break;
        case 7: put_frame(in, 0, noise(4), good, false); break;
        case 8: put_frame(in, 1, noise(8), good, false); break;
        case 9: put_frame(in, 0, noise(4), good, false); break;
        case 10: put_frame(in, 1, {0x50, 0x00}, good, true); break;
        case 11: put_frame(in, (int)below(2), noise(1 + below(20)), good, below(2) != 0); break;
        case 12: put_frame(in, 1, {0x30, (uint8_t)rnd()}, good, true); break;
        default: put_frame(in, 0, noise(16), good, true); break;
        }
    }
    return in;
}

static bool read_routes(const char *path, std::vector<Input> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    for (;;) {
        uint64_t head[3];
        if (fread(head, 8, 3, f) != 3) break;
        Input in;
        in.keyed = true;
        bool ok = fread(&in.st, sizeof in.st, 1, f) == 1 && fread(&in.table, sizeof in.table, 1, f) == 1;
        in.frames.resize(head[0]);
        ok = ok && (head[0] == 0 || fread(in.frames.data(), sizeof(nfc_raw_frame), head[0], f) == head[0]);
        for (int t = 0; t < 2 && ok; t++) {
            in.bytes[t].resize(head[1 + t]), in.par[t].resize(head[1 + t]);
            ok = head[1 + t] == 0 || (fread(in.bytes[t].data(), 1, head[1 + t], f) == head[1 + t] && fread(in.par[t].data(), 1, head[1 + t], f) == head[1 + t]);
        }
        if (!ok) {
            fclose(f);
            return false;
        }
        out.push_back(in);
    }
    fclose(f);
    return true;
}

int main(int argc, char **argv) {
    // 1. the rendered routes
    std::vector<Input> routes;
    if (argc > 1) {
        if (!read_routes(argv[1], routes) || routes.size() != 3) return fail("cannot read three routes from the file");
        nfc_ctx_command_counters cn[3];
        memset(cn, 0, sizeof cn);
        for (size_t r = 0; r < routes.size(); r++)
            for (size_t cut = 0; cut <= routes[r].frames.size(); cut++)
                if (check(routes[r], cut, cut == 0 ? &cn[r] : nullptr)) return fail("route", (long)r);
        if (cn[0].n_segments != 2 || cn[0].n_rerun_segments != 0) return fail("route (a): not two segments, none walked again");
        if (cn[1].n_segments != 4 || cn[1].n_rerun_segments != 3 || cn[1].n_rerun_frames != 57) return fail("route (b): not every later segment walked again");
        if (cn[2].n_keydep_segments < 1 || cn[2].n_rerun_segments != 1) return fail("route (c): the carried cur_key was not read");
        printf("ctx_commands_check: routes %zu\n", routes.size());
    } else {
        printf("ctx_commands_check: routes 0 (no file named: tests/test_ctx_commands_host.py writes one)\n");
    }
    // 2. random lists
    nfc_ctx_command_counters total;
    memset(&total, 0, sizeof total);
    const int lists = 10000;
    for (int i = 0; i < lists; i++) {
        const Input in = random_input();
        if (check(in, in.frames.empty() ? 0 : below((uint32_t)in.frames.size() + 1), &total)) return fail("random list", i);
    }
    printf("ctx_commands_check: random lists %d: %u segments, %u walked again (%u frames), %u read the carried cur_key\n", lists, total.n_segments,
           total.n_rerun_segments, total.n_rerun_frames, total.n_keydep_segments);
    if (total.n_segments < (uint32_t)lists || total.n_rerun_segments == 0 || total.n_keydep_segments == 0)
        return fail("the random lists do not take every route");
    // 3. arguments
    nfc_fsm_state st;
    nfc_fsm_state_init(&st);
    if (nfc_host_commands_segmented(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr) != NFC_ERR_ARG)
        return fail("a null state was accepted");
    if (nfc_host_commands_segmented(&st, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 2, nullptr) != NFC_ERR_ARG)
        return fail("an order without entries was accepted");
    st.cur_cmd = 99;
    if (nfc_host_commands_segmented(&st, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr) != NFC_ERR_ARG)
        return fail("a state out of range was accepted");
    printf("ctx_commands_check: ok\n");
    return 0;
}
