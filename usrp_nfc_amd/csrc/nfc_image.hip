// nfc_image.hip -- the CPU twin of k_multi_images (image.hip.h says what both compute, DESIGN.md 8p why): nfc_card_image_init and
// nfc_host_card_image, in a translation unit of their own so that a stand-alone host program links them without the contexts
// (tools/image_check).  The kernel and the device calls are nfc_multi.hip's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/nfc_amd.h"
#include "image.hip.h"

using namespace nfc;

extern "C" {

int nfc_card_image_init(nfc_card_image *image) {
    if (!image) return NFC_ERR_ARG;
    image::image_init(*image);
    return NFC_OK;
}

int nfc_host_card_image(nfc_card_image *image, const nfc_frame *cmds, size_t n, const uint8_t *data, size_t data_len, const uint8_t key_a[6],
                        const uint8_t key_b[6], const nfc_fsm_key_table *table) {
    if (!image || !key_a || !key_b || (n && !cmds) || (data_len && !data)) return NFC_ERR_ARG;
    if (image::image_fault(*image)) return NFC_ERR_ARG;
    if (table && skeys::table_fault(*table)) return NFC_ERR_ARG;
    const skeys::HostTable keys = {table};
    nfc_card_image g = *image;   // (a record outside `data` leaves the caller's image as it was)
    if (!image::host_run(g, cmds, n, data, data_len, keys, fsmd::key_of(key_a), fsmd::key_of(key_b))) return NFC_ERR_ARG;
    *image = g;
    return NFC_OK;
}

}  // extern "C"
