// keys_check -- nfc_find_auths and nfc_host_recover_keys on the reference vector (the first authentication of
// tests/golden/1k_with_enc.out), then the nested authentication that follows it in that trace: nfc_find_nested_auths, the candidate list
// (nfc_host_nested_candidates) and nfc_host_recover_nested_keys on the one-candidate window of the printed nonce -- the nested verify
// and the host's reduction.  A stand-alone host program: the way to run the key recovery's host code under a sanitizer.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/keys_check/main.cpp \
//         usrp_nfc_amd/csrc/nfc_keys.hip -o keys_check && ./keys_check
// It touches no GPU.  Exit status 0: the frames give the quoted traces, the first one gives key FF FF FF FF FF FF, one candidate, and
// the nested one 64 candidate nonces, 8F 82 69 9E among them, and from that one key FF FF FF FF FF FF with nr 01 3A 6B BA.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nfc_amd.h"
#include "../../usrp_nfc_amd/csrc/protocol.h"

int main() {
    // SEL1R, AUTHA block 0x3C, nt, {nr}{ar}, {at}: reader frames carry type 1
    const uint8_t uid[4] = {0xCD, 0x76, 0x92, 0x74}, nt[4] = {0x0E, 0x61, 0x64, 0xD6};
    const uint8_t nrar[8] = {0x78, 0x5A, 0x41, 0x80, 0x50, 0x04, 0x8F, 0x22}, at[4] = {0xCE, 0xCA, 0x0D, 0x83};
    // the ninth bits of {nr}{ar} and {at} as the trace prints them ('!': the parity bit equals the data parity)
    const int nrar_bang[8] = {0, 0, 0, 1, 1, 1, 0, 1}, at_bang[4] = {1, 1, 1, 0};
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
    add(1, sel, 9, nullptr, NFC_RAW_PARITY_OK | NFC_RAW_CRC_A_OK);
    add(1, auth, 4, nullptr, NFC_RAW_PARITY_OK | NFC_RAW_CRC_A_OK);
    add(0, nt, 4, nullptr, NFC_RAW_PARITY_OK);
    add(1, nrar, 8, nrar_bang, 0);
    add(0, at, 4, at_bang, 0);
    nfc_auth_trace t[2];
    size_t n = 0;
    if (nfc_find_auths(fr.data(), fr.size(), b[0].data(), p[0].data(), b[1].data(), p[1].data(), t, 2, &n) != NFC_OK || n != 1) {
        printf("nfc_find_auths: %zu traces\n", n);
        return 1;
    }
    if (t[0].uid != 0x749276CDu || t[0].nt != 0xD664610Eu || t[0].nr_enc != 0x80415A78u || t[0].ar_enc != 0x228F0450u || t[0].at_enc != 0x830DCACEu ||
        t[0].key_type != 0x60 || t[0].block != 0x3C || t[0].frame != 1 || t[0].idx != 2000) {
        printf("nfc_find_auths: another trace than the quoted one\n");
        return 1;
    }
    nfc_key_result r;
    nfc_key_stats s;
    if (nfc_host_recover_keys(t, 1, nullptr, &r, &s) != NFC_OK) return 1;
    printf("status %d key %02X %02X %02X %02X %02X %02X candidates %u n_odd %u n_even %u nr %08X par %03X\n", r.status, r.key[0], r.key[1], r.key[2], r.key[3],
           r.key[4], r.key[5], r.n_candidates, r.n_odd, r.n_even, r.nr, t[0].par);
    const uint8_t ff[6] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
    if (!(r.status == NFC_KEY_OK && r.n_candidates == 1 && memcmp(r.key, ff, 6) == 0)) return 1;

    // the nested authentication behind it: {AUTHA 0x38}, {nt}, {nr}{ar}, {at} as the trace prints them
    const uint8_t auth2[4] = {0xC6, 0xDC, 0xBA, 0x11}, nt2[4] = {0x70, 0xBD, 0xED, 0x81};
    const uint8_t nrar2[8] = {0xFC, 0x1A, 0x1A, 0x1D, 0x7D, 0x90, 0x7E, 0x24}, at2[4] = {0x87, 0x4D, 0xFF, 0x8A};
    const int auth2_bang[4] = {0, 0, 1, 1}, nt2_bang[4] = {1, 0, 1, 0}, nrar2_bang[8] = {1, 0, 1, 1, 1, 0, 1, 1}, at2_bang[4] = {0, 0, 1, 0};
    add(1, auth2, 4, auth2_bang, 0);
    add(0, nt2, 4, nt2_bang, 0);
    add(1, nrar2, 8, nrar2_bang, 0);
    add(0, at2, 4, at2_bang, 0);
    nfc_nested_trace nest[2];
    if (nfc_find_nested_auths(fr.data(), fr.size(), b[0].data(), p[0].data(), b[1].data(), p[1].data(), nest, 2, &n) != NFC_OK || n != 1) {
        printf("nfc_find_nested_auths: %zu traces\n", n);
        return 1;
    }
    if (nfc_find_auths(fr.data(), fr.size(), b[0].data(), p[0].data(), b[1].data(), p[1].data(), t, 2, &n) != NFC_OK || n != 1) return 1;
    if (nest[0].uid != 0x749276CDu || nest[0].nt_enc != 0x81EDBD70u || nest[0].nr_enc != 0x1D1A1AFCu || nest[0].ar_enc != 0x247E907Du ||
        nest[0].at_enc != 0x8AFF4D87u || nest[0].key_type != 0 || nest[0].block != 0xFF || nest[0].frame != 5 || nest[0].idx != 6000) {
        printf("nfc_find_nested_auths: another trace than the quoted one\n");
        return 1;
    }
    uint32_t cand[64];
    size_t nc = 0, at_i = 64;
    if (nfc_host_nested_candidates(&nest[0], cand, 64, &nc) != NFC_OK || nc != 64) {
        printf("nfc_host_nested_candidates: %zu candidates\n", nc);
        return 1;
    }
    for (size_t i = 0; i < nc; i++) {
        if (i && (cand[i] & 0xFFFFu) <= (cand[i - 1] & 0xFFFFu)) return 1;   // ascending in seed
        if (cand[i] == 0x9E69828Fu) at_i = i;
    }
    if (at_i == 64) {
        printf("the printed nonce is not among the candidates\n");
        return 1;
    }
    nfc_nested_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.cand_first = (uint32_t)at_i, cfg.cand_count = 1;
    nfc_nested_result nres;
    if (nfc_host_recover_nested_keys(nest, 1, &cfg, &nres, &s) != NFC_OK) return 1;
    printf("nested: status %d key %02X %02X %02X %02X %02X %02X verified %u n_nt %u searched %u nt %08X nr %08X n_odd %llu n_even %llu par %04X\n", nres.status,
           nres.key[0], nres.key[1], nres.key[2], nres.key[3], nres.key[4], nres.key[5], nres.n_verified, nres.n_nt, nres.n_searched, nres.nt, nres.nr,
           (unsigned long long)nres.n_odd, (unsigned long long)nres.n_even, nest[0].par);
    if (!(nres.status == NFC_KEY_OK && nres.n_verified == 1 && nres.n_nt == 64 && nres.n_searched == 1 && memcmp(nres.key, ff, 6) == 0 &&
          nres.nt == 0x9E69828Fu && nres.nr == 0xBA6B3A01u))
        return 1;
    // the window beside it holds no key, and one behind the list nothing to search
    cfg.cand_first = (uint32_t)((at_i + 1) % 64);
    if (nfc_host_recover_nested_keys(nest, 1, &cfg, &nres, &s) != NFC_OK || nres.status != NFC_KEY_NONE || nres.n_searched != 1) return 1;
    cfg.cand_first = 64;
    if (nfc_host_recover_nested_keys(nest, 1, &cfg, &nres, &s) != NFC_OK || nres.status != NFC_KEY_NONE || nres.n_searched != 0 || nres.n_nt != 64) return 1;
    cfg.cand_first = 65;
    return nfc_host_recover_nested_keys(nest, 1, &cfg, &nres, &s) == NFC_ERR_ARG ? 0 : 1;
}
