// Host-side checks of csrc/yuv_io.hip under a sanitizer, without a GPU: every call below is refused by the argument validation (-22)
// before any HIP call, so only the entry points' host code runs -- the validation loops over the descriptor arrays included.  Built
// together with the file under test, host code instrumented:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         lossy-vae_amd/csrc/yuv_io.hip tests/c_client/yuv_args_check.cpp -o yuv_args_check && ./yuv_args_check
// The pointer VALUES handed over are never dereferenced on the host (they stand for device addresses); the ARRAYS that hold them are
// real and exactly as long as the entry points may read, so an over-read of one shows up as a sanitizer report.  Exit 0 and "ok" = clean.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lvae_hip.h"

static int fails = 0;
#define EXPECT22(call)                                                      \
    do {                                                                    \
        const int rc_ = (call);                                             \
        if (rc_ != -22) { std::printf("line %d: rc %d\n", __LINE__, rc_); ++fails; } \
    } while (0)

int main() {
    uint8_t* const dev = reinterpret_cast<uint8_t*>(uintptr_t{1} << 20);   // a stand-in for a device address
    float* const fdev = reinterpret_cast<float*>(uintptr_t{1} << 21);
    for (int B : {1, 3, 17, 33}) {                                          // 17, 33: more than one launch chunk of descriptors
        std::vector<const uint8_t*> y(B, dev), u(B, dev), v(B, dev);
        std::vector<uint8_t*> yo(B, dev), uo(B, dev), vo(B, dev);
        std::vector<long> yr(B, 64), ur(B, 32), vr(B, 32);
        std::vector<int> hw(2 * B, 8);
        // the LAST frame is the bad one: the validation walks every array to its end before it refuses
        hw[2 * B - 1] = 7;                                                  // odd width
        EXPECT22(lvae_image_yuv420_to_f32(y.data(), u.data(), v.data(), yr.data(), ur.data(), vr.data(), hw.data(), B, LVAE_YUV_I420, LVAE_YUV_BT709,
                                          LVAE_YUV_LIMITED, LVAE_YUV_BILINEAR, fdev, 3L * 64 * 64, 64, 64, nullptr));
        EXPECT22(lvae_image_f32_to_yuv420(fdev, 3L * 64 * 64, 64 * 64, 64, 64, 64, hw.data(), B, LVAE_YUV_I420, LVAE_YUV_BT709, LVAE_YUV_LIMITED,
                                          yo.data(), uo.data(), vo.data(), yr.data(), ur.data(), vr.data(), nullptr));
        hw[2 * B - 1] = 8;
        vr[B - 1] = 3;                                                      // a chroma row shorter than w / 2
        EXPECT22(lvae_image_yuv420_to_f32(y.data(), u.data(), v.data(), yr.data(), ur.data(), vr.data(), hw.data(), B, LVAE_YUV_I420, LVAE_YUV_BT601,
                                          LVAE_YUV_FULL, LVAE_YUV_NEAREST, fdev, 3L * 64 * 64, 64, 64, nullptr));
        EXPECT22(lvae_image_f32_to_yuv420(fdev, 3L * 64 * 64, 64 * 64, 64, 64, 64, hw.data(), B, LVAE_YUV_I420, LVAE_YUV_BT601, LVAE_YUV_FULL,
                                          yo.data(), uo.data(), vo.data(), yr.data(), ur.data(), vr.data(), nullptr));
        vr[B - 1] = 32;
        ur[B - 1] = 7;                                                      // NV12: v / v_row are not read (null), the UV row holds w bytes
        EXPECT22(lvae_image_yuv420_to_f32(y.data(), u.data(), nullptr, yr.data(), ur.data(), nullptr, hw.data(), B, LVAE_YUV_NV12, LVAE_YUV_BT709,
                                          LVAE_YUV_LIMITED, LVAE_YUV_BILINEAR, fdev, 3L * 64 * 64, 64, 64, nullptr));
        EXPECT22(lvae_image_f32_to_yuv420(fdev, 3L * 64 * 64, 64 * 64, 64, 64, 64, hw.data(), B, LVAE_YUV_NV12, LVAE_YUV_BT709, LVAE_YUV_LIMITED,
                                          yo.data(), uo.data(), nullptr, yr.data(), ur.data(), nullptr, nullptr));
        ur[B - 1] = 32;
        u[B - 1] = nullptr;                                                 // a null entry of a plane array
        uo[B - 1] = nullptr;
        EXPECT22(lvae_image_yuv420_to_f32(y.data(), u.data(), v.data(), yr.data(), ur.data(), vr.data(), hw.data(), B, LVAE_YUV_I420, LVAE_YUV_BT709,
                                          LVAE_YUV_LIMITED, LVAE_YUV_BILINEAR, fdev, 3L * 64 * 64, 64, 64, nullptr));
        EXPECT22(lvae_image_f32_to_yuv420(fdev, 3L * 64 * 64, 64 * 64, 64, 64, 64, hw.data(), B, LVAE_YUV_I420, LVAE_YUV_BT709, LVAE_YUV_LIMITED,
                                          yo.data(), uo.data(), vo.data(), yr.data(), ur.data(), vr.data(), nullptr));
        u[B - 1] = dev;
        uo[B - 1] = dev;
        // everything valid but an enum, a stride or the canvas
        EXPECT22(lvae_image_yuv420_to_f32(y.data(), u.data(), v.data(), yr.data(), ur.data(), vr.data(), hw.data(), B, 2, LVAE_YUV_BT709, LVAE_YUV_LIMITED,
                                          LVAE_YUV_BILINEAR, fdev, 3L * 64 * 64, 64, 64, nullptr));
        EXPECT22(lvae_image_yuv420_to_f32(y.data(), u.data(), v.data(), yr.data(), ur.data(), vr.data(), hw.data(), B, LVAE_YUV_I420, LVAE_YUV_BT709,
                                          LVAE_YUV_LIMITED, 2, fdev, 3L * 64 * 64, 64, 64, nullptr));
        EXPECT22(lvae_image_yuv420_to_f32(y.data(), u.data(), v.data(), yr.data(), ur.data(), vr.data(), hw.data(), B, LVAE_YUV_I420, LVAE_YUV_BT709,
                                          LVAE_YUV_LIMITED, LVAE_YUV_BILINEAR, fdev, 3L * 64 * 64, 4, 64, nullptr));          // extents beyond H
        EXPECT22(lvae_image_f32_to_yuv420(fdev, 3L * 64 * 64, 64 * 64, 63, 64, 64, hw.data(), B, LVAE_YUV_I420, LVAE_YUV_BT709, LVAE_YUV_LIMITED,
                                          yo.data(), uo.data(), vo.data(), yr.data(), ur.data(), vr.data(), nullptr));
        EXPECT22(lvae_image_f32_to_yuv420(fdev, 3L * 64 * 64, 64 * 64, 64, 64, 64, hw.data(), B, LVAE_YUV_I420, 7, LVAE_YUV_LIMITED, yo.data(),
                                          uo.data(), vo.data(), yr.data(), ur.data(), vr.data(), nullptr));
        // lvae_sse_u8: the last pair is the bad one
        std::vector<const uint8_t*> a(B, dev), b(B, dev);
        std::vector<long> ar(B, 8), br(B, 8);
        uint64_t* const out = reinterpret_cast<uint64_t*>(uintptr_t{1} << 22);
        hw[2 * B - 2] = 0;                                                  // a plane of 0 rows
        EXPECT22(lvae_sse_u8(a.data(), ar.data(), b.data(), br.data(), hw.data(), B, out, nullptr));
        hw[2 * B - 2] = 8;
        br[B - 1] = 7;
        EXPECT22(lvae_sse_u8(a.data(), ar.data(), b.data(), br.data(), hw.data(), B, out, nullptr));
        br[B - 1] = 8;
        b[B - 1] = nullptr;
        EXPECT22(lvae_sse_u8(a.data(), ar.data(), b.data(), br.data(), hw.data(), B, out, nullptr));
        b[B - 1] = dev;
        EXPECT22(lvae_sse_u8(a.data(), ar.data(), b.data(), br.data(), hw.data(), B, nullptr, nullptr));
        hw[0] = 2147483647; hw[1] = 2147483647; ar[0] = br[0] = 2147483647;  // a grid beyond what a launch can index
        EXPECT22(lvae_sse_u8(a.data(), ar.data(), b.data(), br.data(), hw.data(), B, out, nullptr));
    }
    EXPECT22(lvae_image_yuv420_to_f32(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0, 0, 0, 0, fdev, 0, 64, 64, nullptr));
    EXPECT22(lvae_image_f32_to_yuv420(nullptr, 0, 0, 0, 64, 64, nullptr, 1, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    EXPECT22(lvae_sse_u8(nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr));
    std::printf(fails ? "FAILED %d\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
