// keys_check -- nfc_find_auths and nfc_host_recover_keys on the reference vector (the first authentication of
// tests/golden/1k_with_enc.out), as a stand-alone host program: the way to run the key recovery's host code under a sanitizer.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/keys_check/main.cpp \
//         usrp_nfc_amd/csrc/nfc_keys.hip -o keys_check && ./keys_check
// It touches no GPU.  Exit status 0: the frames give the quoted trace and the trace gives key FF FF FF FF FF FF, one candidate.
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
    return (r.status == NFC_KEY_OK && r.n_candidates == 1 && memcmp(r.key, ff, 6) == 0) ? 0 : 1;
}
