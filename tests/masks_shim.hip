// The annotator's label-mask kernel on id planes the test supplies: rope_render_masks only ever feeds it planes it has just
// rendered, and an entry point of its own in rope_abi.hip would change rope_build_id.  Built by tests/test_gpu_label_masks.py
// with build.HIPCC_FLAGS into a temporary directory; never part of librope_hip.so.
#include "../rope_s3d_amd/csrc/rope_masks.hip"

extern "C" int shim_label_masks(const uint8_t *ids, int n, int H, int W, const uint8_t *lut, int pad, uint8_t *masks, int32_t *boxes,
                                void *stream)
{
    return (int)rope::launch_masks((hipStream_t)stream, ids, n, H, W, lut, pad, masks, boxes);
}
