// protocol.h -- the host machine behind nfc_fsm_* (fsm.fsm in Python): a thin shell over THE protocol machine of fsm.hip.h.  It adds what
// only the host has: a UID that grows without bound (the reference's list; the kernel's eight words stop at 32 bytes), the per-sector
// key table held beside the machine, the packet entry (the frame is assembled here, by the text the GPU assembles it with) and
// fsm.process_outgoing for an emulator.  No command table, no lookup and no cipher of its own.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/nfc_amd.h"
#include "frames.hip.h"
#include "fsm.hip.h"
#include "sector_keys.h"

// (the Machine's eight UID words and its flags stay empty: the UID is `uid`, and nothing is lost or cut here)
struct nfc_fsm : nfc::fsmd::Machine {
    nfc_fsm() { nfc::fsmd::machine_init(*this); }
    std::vector<uint8_t> uid;
    nfc_fsm_key_table table = {};   // the per-sector keys; empty: the two keys of the Machine serve every sector
    std::vector<uint8_t> raw;       // scratch of the packet entry: a frame's bytes and ninth bits as received
    std::vector<uint16_t> enc;      // ... and its enc entries where the caller wants none
};

namespace nfc {
namespace fsmd {
// the unbounded UID holder (fsm.hip.h: the accessor).  Host only: nothing the device instantiates may name an nfc_fsm.
inline uint32_t uid_len(const nfc_fsm &F) { return (uint32_t)F.uid.size(); }
inline uint32_t uid_byte(const nfc_fsm &F, uint32_t i) { return i < F.uid.size() ? F.uid[i] : 0u; }
inline void uid_clear(nfc_fsm &F) { F.uid.clear(); }
inline void uid_append(nfc_fsm &F, const Bytes &B, uint32_t from, uint32_t n) {
    for (uint32_t j = 0; j < n; j++) F.uid.push_back((uint8_t)B.at(from + j));
}
}  // namespace fsmd
// ALL FOUR must stay overloaded together, and the core (fsm.hip.h) must reach the UID through them alone: a call with no overload for
// nfc_fsm binds, silently, to the capped Machine's (nfc_fsm_set_state uses exactly that binding to clear the words it does not use).

// frames::ByteBits for the host's packet entry: a whole field's eight data bits are gathered by one 64-bit load and a multiply (byte j's
// bit 0 to bit 56 + j; no two products meet, so nothing carries) where ByteBits makes nine loads.  Little-endian hosts.
struct HostByteBits {
    const uint8_t *b;
    uint32_t field(uint64_t pos, uint64_t end) const {
        if (end - pos < 9) return frames::ByteBits{b}.field(pos, end);
        uint64_t x;
        memcpy(&x, b + pos, 8);
        return (uint32_t)(((x & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56) | (uint32_t)(b[pos + 8] & 1u) << 8;
    }
};

// One frame as the GPU assembled it (nfc_raw_frame: csrc/frames.hip.h; not a cut one).  bytes_out receives the frame's bytes, enc_out
// (optional) its enc entries while a session is up; both are written for all of the raw n_bytes (capacity >= n_bits / 9 + 1 covers that).
inline void fsm_process_frame(nfc_fsm &F, int type, uint32_t raw_flags, uint32_t n, const uint8_t *bytes, const uint8_t *par, nfc_frame *out,
                              uint8_t *bytes_out, uint16_t *enc_out = nullptr) {
    if (!enc_out) {
        if (F.enc.size() < n) F.enc.resize(n);
        enc_out = F.enc.data();
    }
    const fsmd::Rec r = fsmd::process_frame(F, type, raw_flags, n, bytes, par, bytes_out, enc_out, skeys::HostTable{&F.table});
    memset(out, 0, sizeof *out);
    out->cmd = r.cmd, out->type = r.type, out->flags = r.flags;
    out->n_bytes = (uint16_t)r.n_bytes, out->n_header = (uint16_t)r.n_header, out->n_extra = (uint16_t)r.n_extra;
    out->n_crc = (uint16_t)r.n_crc, out->n_enc = (uint16_t)r.n_enc;
}

// One packet (bits as PacketProcessor hands them over, packets.py:94-98): assembled as the frame kernels assemble it -- the repair of the
// frame end, nine bits to a byte, parity and CRC_A (frames.hip.h) -- and then the frame's way.
inline void fsm_process(nfc_fsm &F, const uint8_t *bits, size_t n_bits, int type, nfc_frame *out, uint8_t *bytes_out, uint16_t *enc_out = nullptr) {
    const uint32_t n = frames::frame_bytes_of((uint32_t)n_bits);
    if (F.raw.size() < 2 * (size_t)n) F.raw.resize(2 * (size_t)n);
    uint8_t *b = F.raw.data(), *p = b + n;
    const uint32_t flags = frames::assemble_frame(HostByteBits{bits}, 0, (uint32_t)n_bits, type, n, b, p);
    fsm_process_frame(F, type, flags, n, b, p, out, bytes_out, enc_out);
}

// fsm.process_outgoing (fsm.py:68-112): what an EMULATOR is about to send, the frame's bits (parity bits included, as the encoders take
// them) in, the bits to put on the air out: fsmd::outgoing over the two bit lists, the reference's hook (not NFC_EMU_CARD's).  Returns 1
// when the tag is an Ultralight: the reference then runs the frame through process_bits "to update state" (fsm.py:71-72) -- the caller
// does, with its callback.
struct BitListOut {
    uint8_t *o;
    void operator()(size_t k, uint32_t v) { o[k] = (uint8_t)(v & 1u); }
};
inline int fsm_process_outgoing(nfc_fsm &M, const uint8_t *bits, size_t n, int cmd, uint8_t *out) {
    BitListOut o = {out};
    return fsmd::outgoing(M, n, cmd, [bits](size_t k) { return (uint32_t)bits[k]; }, o, skeys::HostTable{&M.table}, false);
}

}  // namespace nfc
