// reader_keys_check -- nfc_find_reader_auths and nfc_host_recover_reader_keys on two reader-side first authentications of key
// FF FF FF FF FF FF: the reference vector (the first authentication of tests/golden/1k_with_enc.out) WITHOUT its {at}, and a second
// session of the same card made with the project's machine (nt 01 20 01 45, nr 00 00 00 00), which ends the frame list after {nr}{ar}.
// A stand-alone host program: the way to run the reader-pair recovery's host code under a sanitizer.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/reader_keys_check/main.cpp \
//         usrp_nfc_amd/csrc/nfc_keys.hip -o reader_keys_check && ./reader_keys_check
// It touches no GPU.  Exit status 0: the frames give the two quoted traces (and nfc_find_auths only the first, which has an {at}); the
// pair gives key FF FF FF FF FF FF, one candidate of 67 325 joined, n_odd 446 989, n_even 634 554, nr 15 45 90 A8 and 00 00 00 00; one
// flipped bit of the check session's {ar} gives NFC_KEY_NONE; the searched session twice gives NFC_KEY_AMBIGUOUS; a table limit of 2^16
// slots gives NFC_KEY_OVERFLOW with the same counts; a bad key type and an unknown flag are NFC_ERR_ARG.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nfc_amd.h"
#include "../../usrp_nfc_amd/csrc/protocol.h"

int main() {
    const uint8_t uid[4] = {0xCD, 0x76, 0x92, 0x74};
    const uint8_t nt[4] = {0x0E, 0x61, 0x64, 0xD6}, nrar[8] = {0x78, 0x5A, 0x41, 0x80, 0x50, 0x04, 0x8F, 0x22}, at[4] = {0xCE, 0xCA, 0x0D, 0x83};
    const uint8_t nt2[4] = {0x01, 0x20, 0x01, 0x45}, nrar2[8] = {0x64, 0x60, 0x9F, 0xC0, 0x23, 0x3D, 0x5C, 0x58};
    // the ninth bits ('!' in the reference's print: the parity bit equals the data parity)
    const int nrar_bang[8] = {0, 0, 0, 1, 1, 1, 0, 1}, at_bang[4] = {1, 1, 1, 0}, nrar2_bang[8] = {1, 1, 0, 0, 1, 0, 0, 0};
    std::vector<uint8_t> b[2], p[2];
    std::vector<nfc_raw_frame> fr;
    auto add = [&](int type, const uint8_t *d, size_t n, const int *bang, uint32_t flags) {
        nfc_raw_frame r;
        memset(&r, 0, sizeof r);
        r.idx = 1000 * (fr.size() + 1), r.byte_off = (uint32_t)b[type].size(), r.n_bits = (uint32_t)(9 * n), r.n_bytes = (uint32_t)n;
        r.flags = flags, r.type = type;
        for (size_t i = 0; i < n; i++) {
            const int ones = __builtin_popcount(d[i]) & 1;
            b[type].push_back(d[i]);
            p[type].push_back((uint8_t)(bang ? (bang[i] ? ones : 1 - ones) : 1 - ones));
        }
        fr.push_back(r);
    };
    uint8_t sel[9] = {0x93, 0x70, uid[0], uid[1], uid[2], uid[3], (uint8_t)(uid[0] ^ uid[1] ^ uid[2] ^ uid[3]), 0, 0};
    uint16_t c = nfc::crc_a(sel, 7);
    sel[7] = (uint8_t)c, sel[8] = (uint8_t)(c >> 8);
    uint8_t auth[4] = {0x60, 0x3C, 0, 0};
    c = nfc::crc_a(auth, 2);
    auth[2] = (uint8_t)c, auth[3] = (uint8_t)(c >> 8);
    const uint32_t good = NFC_RAW_PARITY_OK | NFC_RAW_CRC_A_OK;
    add(1, sel, 9, nullptr, good);
    add(1, auth, 4, nullptr, good);
    add(0, nt, 4, nullptr, NFC_RAW_PARITY_OK);
    add(1, nrar, 8, nrar_bang, 0);
    add(0, at, 4, at_bang, 0);
    add(1, sel, 9, nullptr, good);
    add(1, auth, 4, nullptr, good);
    add(0, nt2, 4, nullptr, NFC_RAW_PARITY_OK);
    add(1, nrar2, 8, nrar2_bang, 0);   // the list ends here: no {at}
    nfc_auth_trace t[3], full[3];
    size_t n = 0, n_full = 0;
    if (nfc_find_reader_auths(fr.data(), fr.size(), b[0].data(), p[0].data(), b[1].data(), p[1].data(), t, 3, &n) != NFC_OK || n != 2 ||
        nfc_find_auths(fr.data(), fr.size(), b[0].data(), p[0].data(), b[1].data(), p[1].data(), full, 3, &n_full) != NFC_OK || n_full != 1) {
        printf("nfc_find_reader_auths: %zu traces, nfc_find_auths: %zu\n", n, n_full);
        return 1;
    }
    if (t[0].uid != 0x749276CDu || t[0].nt != 0xD664610Eu || t[0].nr_enc != 0x80415A78u || t[0].ar_enc != 0x228F0450u || t[0].at_enc != 0 || t[0].par != 0x02F ||
        t[0].key_type != 0x60 || t[0].block != 0x3C || t[0].frame != 1 || t[0].idx != 2000 || full[0].frame != 1 || full[0].at_enc != 0x830DCACEu ||
        t[1].uid != 0x749276CDu || t[1].nt != 0x45012001u || t[1].nr_enc != 0xC09F6064u || t[1].ar_enc != 0x585C3D23u || t[1].at_enc != 0 || t[1].par != 0x05D ||
        t[1].frame != 6 || t[1].idx != 7000) {
        printf("nfc_find_reader_auths: other traces than the quoted ones\n");
        return 1;
    }
    nfc_reader_pair pairs[3];
    pairs[0].search = t[0], pairs[0].check = t[1];
    pairs[1] = pairs[0];
    pairs[1].check.ar_enc ^= 1u << 13;
    pairs[2].search = t[0], pairs[2].check = t[0];
    nfc_reader_key_result r[3];
    nfc_key_stats s;
    if (nfc_host_recover_reader_keys(pairs, 3, nullptr, r, &s) != NFC_OK) return 1;
    for (int i = 0; i < 3; i++)
        printf("pair %d: status %d key %02X %02X %02X %02X %02X %02X candidates %u joined %u n_odd %u n_even %u nr %08X %08X\n", i, r[i].status, r[i].key[0],
               r[i].key[1], r[i].key[2], r[i].key[3], r[i].key[4], r[i].key[5], r[i].n_candidates, r[i].n_joined, r[i].n_odd, r[i].n_even, r[i].nr_search,
               r[i].nr_check);
    const uint8_t ff[6] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
    if (!(r[0].status == NFC_KEY_OK && r[0].n_candidates == 1 && memcmp(r[0].key, ff, 6) == 0 && r[0].n_joined == 67325 && r[0].n_odd == 446989 &&
          r[0].n_even == 634554 && r[0].nr_search == 0xA8904515u && r[0].nr_check == 0))
        return 1;
    if (!(r[1].status == NFC_KEY_NONE && r[1].n_candidates == 0 && r[1].n_joined == 67325)) return 1;
    if (!(r[2].status == NFC_KEY_AMBIGUOUS && r[2].n_candidates > 1 && r[2].nr_search == r[2].nr_check)) return 1;
    if (s.n_batches != 1 || s.n_grown != 0) return 1;

    nfc_reader_key_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.search.max_capacity = 1u << 16;
    if (nfc_host_recover_reader_keys(pairs, 1, &cfg, r, &s) != NFC_OK || r[0].status != NFC_KEY_OVERFLOW || r[0].n_odd != 446989 || r[0].n_even != 634554 ||
        r[0].n_joined != 0 || r[0].n_candidates != 0)
        return 1;
    memset(&cfg, 0, sizeof cfg);
    cfg.flags = 2;
    if (nfc_host_recover_reader_keys(pairs, 1, &cfg, r, &s) != NFC_ERR_ARG) return 1;
    pairs[0].check.key_type = 0x30;
    if (nfc_host_recover_reader_keys(pairs, 1, nullptr, r, &s) != NFC_ERR_ARG) return 1;
    return nfc_host_recover_reader_keys(pairs, 0, nullptr, nullptr, nullptr) == NFC_OK ? 0 : 1;
}
