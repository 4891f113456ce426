// emu_check -- the two host twins of the emulation (include/nfc_amd.h: nfc_host_emu_step, nfc_host_emulate, nfc_host_emulate_pairs; csrc/emu.hip.h,
// DESIGN.md 8k) over cards made here: a Classic 1K with sixteen different key pairs read by a reader with the full table, the blank
// card of Tag.generate_1k, and an Ultralight -- both links, both modes, two rounds, in slabs of the exact size and in slabs that are
// outgrown.  A stand-alone host program: the way to run the emulators' host code under a sanitizer.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/emu_check/main.cpp \
//         usrp_nfc_amd/csrc/nfc_emu.hip usrp_nfc_amd/csrc/nfc_commands.hip -o emu_check && ./emu_check
// It touches no GPU.  Exit status 0: every whole-card read has 199 frames a round and no flag; a slab that is outgrown holds a prefix
// of the whole transcript and the true counts; a step-by-step read through nfc_host_emu_step sends the loop's plain frames; a replay
// through nfc_host_emulate in either role, whole and in two pieces, puts the transcript's frames on the air.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nfc_amd.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

struct Cards {
    std::vector<uint8_t> mem, tag_rands, reader_rands;
    nfc_fsm_key_table table;
    nfc_emu_card tag, reader;
};
// kind 0: sixteen key pairs; 1: the blank card (FF keys); 2: an Ultralight
static void make(Cards &c, int kind, int mode, uint32_t seed) {
    memset(&c.tag, 0, sizeof c.tag), memset(&c.reader, 0, sizeof c.reader);
    nfc_fsm_key_table_init(&c.table);
    c.mem.assign(kind == 2 ? 64 : 1024, 0);
    for (auto &b : c.mem) b = (uint8_t)(lcg(seed) >> 24);
    if (kind != 2) {
        c.mem[4] = c.mem[0] ^ c.mem[1] ^ c.mem[2] ^ c.mem[3];
        for (int s = 0; s < 16; s++) {
            uint8_t *t = c.mem.data() + (4 * s + 3) * 16;
            if (kind == 1) memset(t, 0xFF, 16);
            t[6] = 0xFF, t[7] = 0x07, t[8] = 0x80, t[9] = 0x69;   // the transport configuration: data blocks free, key B readable
            memcpy(c.table.key[0][s], t, 6), c.table.present[0][s] = 1;
        }
    } else {
        c.mem[3] = 0x88 ^ c.mem[0] ^ c.mem[1] ^ c.mem[2];
        c.mem[8] = c.mem[4] ^ c.mem[5] ^ c.mem[6] ^ c.mem[7];
    }
    c.tag_rands.assign(4 * 5, 0), c.reader_rands.assign(4 * 3, 0);
    for (auto &b : c.tag_rands) b = (uint8_t)(lcg(seed) >> 24);
    for (auto &b : c.reader_rands) b = (uint8_t)(lcg(seed) >> 24);
    c.tag.role = NFC_EMU_TAG, c.tag.tag_type = kind == 2 ? 0 : 1, c.tag.mode = mode;
    c.tag.mem = c.mem.data(), c.tag.mem_len = (uint32_t)c.mem.size();
    c.tag.rands = c.tag_rands.data(), c.tag.n_rands = 5;
    c.reader.role = NFC_EMU_READER, c.reader.mode = mode, c.reader.rands = c.reader_rands.data(), c.reader.n_rands = 3;
    memset(c.reader.key_a, 0xFF, 6), memset(c.reader.key_b, 0xFF, 6);
    c.reader.table = kind == 0 ? &c.table : nullptr;
}

struct Run {
    nfc_emu_pair_result res;
    std::vector<nfc_emu_frame> frames;
    std::vector<uint8_t> plain, air, par;
};
static bool run(const Cards &c, uint32_t link, uint32_t rounds, uint32_t cap_frames, uint32_t cap_bytes, Run &r) {
    nfc_emu_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.link = link, cfg.rounds = rounds, cfg.cap_frames = cap_frames, cfg.cap_bytes = cap_bytes;
    r.frames.assign(cap_frames, nfc_emu_frame()), r.plain.assign(cap_bytes, 0), r.air.assign(cap_bytes, 0), r.par.assign(cap_bytes, 0);
    return nfc_host_emulate_pairs(&c.tag, &c.reader, 1, &cfg, &r.res, r.frames.data(), r.plain.data(), r.air.data(), r.par.data()) == NFC_OK;
}

int main() {
    for (int kind = 0; kind < 3; kind++)
        for (int mode = 0; mode < 2; mode++)
            for (uint32_t link = 0; link < 2; link++) {
                Cards c;
                make(c, kind, mode, 1234u + (uint32_t)kind);
                Run probe;
                if (!run(c, link, 2, 1024, 8192, probe)) {
                    printf("kind %d mode %d link %u: nfc_host_emulate_pairs failed: %s\n", kind, mode, link, nfc_emu_last_error());
                    return 1;
                }
                // the reference's hook cannot read a Classic over the air past its first sector (the nested nonce's quirk); a card whose
                // sectors have keys of their own is beyond the reference's tag in any case
                const bool whole = kind == 2 || link == NFC_EMU_LINK_PLAIN || mode == NFC_EMU_CARD;
                const uint32_t want = kind == 2 ? 2 * 19 : 2 * 199;
                if (whole && (probe.res.n_frames != want || probe.res.flags || probe.res.tag_flags || probe.res.reader_flags)) {
                    printf("kind %d mode %d link %u: %u frames, flags %u %u %u\n", kind, mode, link, probe.res.n_frames, probe.res.flags, probe.res.tag_flags,
                           probe.res.reader_flags);
                    return 1;
                }
                // slabs of the exact size (a write past them is a write past a vector's end), then slabs that are outgrown
                Run exact;
                if (!run(c, link, 2, probe.res.n_frames, probe.res.n_bytes, exact) || exact.res.flags ||
                    memcmp(exact.frames.data(), probe.frames.data(), exact.frames.size() * sizeof(nfc_emu_frame)) != 0 ||
                    memcmp(exact.air.data(), probe.air.data(), exact.air.size()) != 0 || memcmp(exact.par.data(), probe.par.data(), exact.par.size()) != 0) {
                    printf("kind %d mode %d link %u: exact slabs give another transcript\n", kind, mode, link);
                    return 1;
                }
                for (int cut = 0; cut < 2; cut++) {
                    Run small;
                    const uint32_t cf = cut ? probe.res.n_frames : 7, cb = cut ? 23 : probe.res.n_bytes;
                    if (!run(c, link, 2, cf, cb, small) || small.res.n_frames != probe.res.n_frames || small.res.n_bytes != probe.res.n_bytes ||
                        small.res.flags != (cut ? NFC_EMU_PAIR_CUT_BYTES : NFC_EMU_PAIR_CUT_FRAMES)) {
                        printf("kind %d mode %d link %u cut %d: counts %u %u flags %u\n", kind, mode, link, cut, small.res.n_frames, small.res.n_bytes, small.res.flags);
                        return 1;
                    }
                    for (uint32_t i = 0; i < cf && small.frames[i].n_bits; i++)
                        if (memcmp(&small.frames[i], &probe.frames[i], sizeof(nfc_emu_frame)) != 0 ||
                            memcmp(small.air.data() + small.frames[i].byte_off, probe.air.data() + probe.frames[i].byte_off, small.frames[i].n_bytes) != 0) {
                            printf("kind %d mode %d link %u cut %d: frame %u is not the whole transcript's\n", kind, mode, link, cut, i);
                            return 1;
                        }
                }
                if (link != NFC_EMU_LINK_PLAIN) continue;
                // the same read step by step: each machine hears the other's plain frame
                nfc_emu_state st, sr;
                nfc_emu_state_init(&st), nfc_emu_state_init(&sr);
                int cmd = probe.frames[0].cmd;
                uint8_t frame[18] = {0x26};
                size_t n = 1;
                bool to_tag = true;
                for (uint32_t i = 0; i + 1 < probe.res.n_frames / 2; i++) {
                    nfc_command_info info;
                    nfc_command_get(cmd, &info);
                    const size_t h = (size_t)info.n_header, ne = n - h - (info.crc ? 2 : 0);
                    int next = -1;
                    uint8_t out[18];
                    size_t n_out = 0;
                    if (nfc_host_emu_step(to_tag ? &c.tag : &c.reader, to_tag ? &st : &sr, cmd, frame + h, ne, &next, out, &n_out) != NFC_OK) {
                        printf("nfc_host_emu_step failed: %s\n", nfc_emu_last_error());
                        return 1;
                    }
                    const nfc_emu_frame &f = probe.frames[i + 1];
                    if (next != f.cmd || n_out != f.n_bytes || memcmp(out, probe.plain.data() + f.byte_off, n_out) != 0) {
                        printf("kind %d mode %d: step %u answers another frame than the loop\n", kind, mode, i);
                        return 1;
                    }
                    cmd = next, n = n_out, memcpy(frame, out, 18), to_tag = !to_tag;
                }
            }
    // replay (nfc_host_emulate): a tag card behind a machine hears the READER frames of its own whole-card transcript, a reader card the
    // tag frames -- what each puts on the air is the transcript's next frame, in one piece and cut in two with the states handed on
    for (int role = 0; role < 2; role++) {
        Cards c;
        make(c, 1, NFC_EMU_CARD, 99);
        Run t;
        if (!run(c, NFC_EMU_LINK_AIR, 1, 256, 2048, t) || t.res.n_frames != 199) return printf("replay: no transcript\n"), 1;
        std::vector<nfc_raw_frame> heard;
        std::vector<int> next;   // per heard frame: the transcript frame that answers it, or -1
        for (uint32_t i = 0; i < t.res.n_frames; i++) {
            const nfc_emu_frame &f = t.frames[i];
            if ((int)f.type == role) continue;
            nfc_raw_frame r;
            memset(&r, 0, sizeof r);
            r.idx = i, r.byte_off = f.byte_off, r.n_bits = f.n_bits == 7 ? 8 : f.n_bits, r.n_bytes = f.n_bytes, r.type = f.type;
            // parity and CRC_A verdicts as the frame assembly gives them
            bool par_ok = true;
            for (uint32_t j = 0; j < f.n_bytes; j++) par_ok = par_ok && ((__builtin_popcount(t.air[f.byte_off + j]) & 1) != (t.par[f.byte_off + j] & 1));
            uint8_t crc[2] = {0, 0};
            if (f.n_bytes > 2) nfc_crc_a(t.air.data() + f.byte_off, f.n_bytes - 2, crc);
            r.flags = par_ok ? NFC_RAW_PARITY_OK : 0;
            if (par_ok && f.n_bytes > 2 && crc[0] == t.air[f.byte_off + f.n_bytes - 2] && crc[1] == t.air[f.byte_off + f.n_bytes - 1]) r.flags |= NFC_RAW_CRC_A_OK;
            heard.push_back(r);
            next.push_back(i + 1 < t.res.n_frames && (int)t.frames[i + 1].type == role ? (int)(i + 1) : -1);
        }
        const nfc_emu_card &card = role == 0 ? c.tag : c.reader;
        for (size_t cut : {heard.size(), (size_t)5, (size_t)9}) {
            nfc_fsm_state st;
            nfc_emu_state est;
            nfc_fsm_state_init(&st), nfc_emu_state_init(&est);
            size_t total = 0, done = 0;
            const size_t edges[3] = {0, cut, heard.size()};
            for (int part = 0; part < 2; part++) {
                const size_t a = edges[part], b = edges[part + 1], m = b - a;
                if (!m) continue;
                size_t room = 0, used = 0, n_ans = 0;
                for (size_t i = a; i < b; i++) room += heard[i].n_bytes;
                std::vector<nfc_frame> out(m);
                std::vector<uint8_t> data(room), ap(18 * m), aa(18 * m), aq(18 * m);
                std::vector<uint16_t> enc(room);
                std::vector<nfc_emu_answer> ans(m);
                if (nfc_host_emulate(&st, nullptr, &card, &est, heard.data() + a, m, t.air.data(), t.par.data(), t.air.data(), t.par.data(), out.data(), data.data(),
                                     enc.data(), room, &used, ans.data(), ap.data(), aa.data(), aq.data(), &n_ans) != NFC_OK || used != room) {
                    printf("replay role %d: nfc_host_emulate failed: %s\n", role, nfc_emu_last_error());
                    return 1;
                }
                for (size_t j = 0; j < n_ans; j++) {
                    const int want = next[a + ans[j].src];
                    if (want < 0) return printf("replay role %d: an answer to a frame the transcript leaves unanswered\n", role), 1;
                    const nfc_emu_frame &f = t.frames[want];
                    if (ans[j].cmd != f.cmd || ans[j].n_bytes != f.n_bytes || memcmp(aa.data() + ans[j].byte_off, t.air.data() + f.byte_off, f.n_bytes) != 0 ||
                        memcmp(aq.data() + ans[j].byte_off, t.par.data() + f.byte_off, f.n_bytes) != 0) {
                        printf("replay role %d cut %zu: answer to heard frame %zu is not the transcript's\n", role, cut, a + ans[j].src);
                        return 1;
                    }
                }
                total += n_ans, done += m;
            }
            if (total != 99 || done != heard.size() || est.flags) return printf("replay role %d cut %zu: %zu answers\n", role, cut, total), 1;
        }
    }
    // the narrowings
    Cards c;
    make(c, 0, NFC_EMU_CARD, 7);
    Run r;
    c.tag.mem_len = 1000;
    if (run(c, NFC_EMU_LINK_AIR, 1, 8, 64, r) || !strstr(nfc_emu_last_error(), "tags[0].mem")) return printf("a short memory was accepted\n"), 1;
    c.tag.mem_len = 1024, c.reader.n_rands = 0;
    if (run(c, NFC_EMU_LINK_AIR, 1, 8, 64, r) || !strstr(nfc_emu_last_error(), "readers[0].rands")) return printf("a reader without nonces was accepted\n"), 1;
    printf("emu_check: ok\n");
    return 0;
}
