// Host-side checks of csrc/yuv_io.hip (all eight entries) under a sanitizer, without a GPU: every call below is refused by the argument
// validation (-22) before any HIP call, so only the entry points' host code runs -- the validation loops over the descriptor arrays included.  Built
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

static uint8_t* const dev = reinterpret_cast<uint8_t*>(uintptr_t{1} << 20);   // a stand-in for a device address
static float* const fdev = reinterpret_cast<float*>(uintptr_t{1} << 21);
static uint64_t* const out = reinterpret_cast<uint64_t*>(uintptr_t{1} << 22);

// lvae_image_yuv_to_f32 / lvae_image_f32_to_yuv: B planar frames, the LAST descriptor the bad one
static void general(int B) {
    std::vector<const void*> y(B, dev), u(B, dev), v(B, dev);
    std::vector<void*> yo(B, dev), uo(B, dev), vo(B, dev);
    std::vector<long> yr(B, 64), ur(B, 32), vr(B, 32);
    std::vector<int> hw(2 * B, 8);
    auto in = [&](int depth, int sub, int siting, int matrix, int chroma, int H) {
        return lvae_image_yuv_to_f32(y.data(), u.data(), v.data(), yr.data(), ur.data(), vr.data(), hw.data(), B, depth, sub, siting, matrix,
                                     LVAE_YUV_LIMITED, chroma, fdev, 3L * 64 * 64, H, 64, nullptr);
    };
    auto back = [&](int depth, int sub, int siting, int matrix, long src_row) {
        return lvae_image_f32_to_yuv(fdev, 3L * 64 * 64, 64 * 64, src_row, 64, 64, hw.data(), B, depth, sub, siting, matrix, LVAE_YUV_FULL, yo.data(),
                                     uo.data(), vo.data(), yr.data(), ur.data(), vr.data(), nullptr);
    };
    hw[2 * B - 1] = 7;                                                      // odd width at 4:2:2
    EXPECT22(in(10, LVAE_YUV_SUB_422, LVAE_YUV_SITING_LEFT, LVAE_YUV_BT2020, LVAE_YUV_BILINEAR, 64));
    EXPECT22(back(10, LVAE_YUV_SUB_422, LVAE_YUV_SITING_LEFT, LVAE_YUV_BT2020, 64));
    hw[2 * B - 1] = 8;
    hw[2 * B - 2] = 7;                                                      // odd height at 4:2:0
    EXPECT22(in(8, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, LVAE_YUV_BT709, LVAE_YUV_NEAREST, 64));
    EXPECT22(back(12, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, LVAE_YUV_BT601, 64));
    hw[2 * B - 2] = 8;
    vr[B - 1] = 7;                                                          // 4:4:4: a chroma row shorter than w
    EXPECT22(in(12, LVAE_YUV_SUB_444, LVAE_YUV_SITING_CENTER, LVAE_YUV_BT709, LVAE_YUV_BILINEAR, 64));
    EXPECT22(back(8, LVAE_YUV_SUB_444, LVAE_YUV_SITING_CENTER, LVAE_YUV_BT709, 64));
    vr[B - 1] = 32;
    v[B - 1] = nullptr;                                                     // a null entry of a plane array
    vo[B - 1] = nullptr;
    EXPECT22(in(8, LVAE_YUV_SUB_420, LVAE_YUV_SITING_LEFT, LVAE_YUV_BT709, LVAE_YUV_BILINEAR, 64));
    EXPECT22(back(8, LVAE_YUV_SUB_420, LVAE_YUV_SITING_LEFT, LVAE_YUV_BT709, 64));
    v[B - 1] = dev;
    vo[B - 1] = dev;
    // everything valid but an enum, a stride or the canvas
    EXPECT22(in(9, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, LVAE_YUV_BT709, LVAE_YUV_BILINEAR, 64));
    EXPECT22(in(8, 3, LVAE_YUV_SITING_CENTER, LVAE_YUV_BT709, LVAE_YUV_BILINEAR, 64));
    EXPECT22(in(8, LVAE_YUV_SUB_420, 2, LVAE_YUV_BT709, LVAE_YUV_BILINEAR, 64));
    EXPECT22(in(8, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, 3, LVAE_YUV_BILINEAR, 64));
    EXPECT22(in(8, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, LVAE_YUV_BT709, 2, 64));
    EXPECT22(in(8, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, LVAE_YUV_BT709, LVAE_YUV_BILINEAR, 4));      // extents beyond H
    EXPECT22(back(16, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, LVAE_YUV_BT709, 64));
    EXPECT22(back(8, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, LVAE_YUV_BT709, 63));
}

// lvae_image_yuvsp_to_f32 / lvae_image_f32_to_yuvsp: B P010-family frames, the LAST descriptor the bad one
static void semiplanar(int B) {
    uint16_t* const wdev = reinterpret_cast<uint16_t*>(dev);
    std::vector<const uint16_t*> y(B, wdev), uv(B, wdev);
    std::vector<uint16_t*> yo(B, wdev), uvo(B, wdev);
    std::vector<long> yr(B, 64), uvr(B, 64);
    std::vector<int> hw(2 * B, 8);
    auto in = [&](int depth, int sub, int siting, int chroma) {
        return lvae_image_yuvsp_to_f32(y.data(), uv.data(), yr.data(), uvr.data(), hw.data(), B, depth, sub, siting, LVAE_YUV_BT2020, LVAE_YUV_LIMITED,
                                       chroma, fdev, 3L * 64 * 64, 64, 64, nullptr);
    };
    auto back = [&](int depth, int sub, int siting) {
        return lvae_image_f32_to_yuvsp(fdev, 3L * 64 * 64, 64 * 64, 64, 64, 64, hw.data(), B, depth, sub, siting, LVAE_YUV_BT709, LVAE_YUV_FULL,
                                       yo.data(), uvo.data(), yr.data(), uvr.data(), nullptr);
    };
    hw[2 * B - 1] = 7;                                                      // odd width
    EXPECT22(in(10, LVAE_YUV_SUB_422, LVAE_YUV_SITING_LEFT, LVAE_YUV_BILINEAR));
    EXPECT22(back(12, LVAE_YUV_SUB_422, LVAE_YUV_SITING_CENTER));
    hw[2 * B - 1] = 8;
    uvr[B - 1] = 7;                                                         // the UV row holds w samples
    EXPECT22(in(12, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, LVAE_YUV_NEAREST));
    EXPECT22(back(10, LVAE_YUV_SUB_420, LVAE_YUV_SITING_LEFT));
    uvr[B - 1] = 64;
    uv[B - 1] = nullptr;                                                    // a null entry of a plane array
    uvo[B - 1] = nullptr;
    EXPECT22(in(10, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, LVAE_YUV_BILINEAR));
    EXPECT22(back(10, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER));
    uv[B - 1] = wdev;
    uvo[B - 1] = wdev;
    // everything valid but the layout: semi-planar frames are 10 / 12 bits at 4:2:0 / 4:2:2
    EXPECT22(in(8, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, LVAE_YUV_BILINEAR));
    EXPECT22(in(10, LVAE_YUV_SUB_444, LVAE_YUV_SITING_CENTER, LVAE_YUV_BILINEAR));
    EXPECT22(in(10, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER, 2));
    EXPECT22(back(8, LVAE_YUV_SUB_420, LVAE_YUV_SITING_CENTER));
    EXPECT22(back(12, LVAE_YUV_SUB_444, LVAE_YUV_SITING_CENTER));
    EXPECT22(back(12, LVAE_YUV_SUB_422, 2));
}

// lvae_sse_u16: the cases of lvae_sse_u8 in main, the last pair the bad one
static void sse_u16(int B) {
    uint16_t* const wdev = reinterpret_cast<uint16_t*>(dev);
    std::vector<const uint16_t*> a(B, wdev), b(B, wdev);
    std::vector<long> ar(B, 8), br(B, 8);
    std::vector<int> hw(2 * B, 8);
    hw[2 * B - 2] = 0;                                                      // a plane of 0 rows
    EXPECT22(lvae_sse_u16(a.data(), ar.data(), b.data(), br.data(), hw.data(), B, out, nullptr));
    hw[2 * B - 2] = 8;
    br[B - 1] = 7;
    EXPECT22(lvae_sse_u16(a.data(), ar.data(), b.data(), br.data(), hw.data(), B, out, nullptr));
    br[B - 1] = 8;
    b[B - 1] = nullptr;
    EXPECT22(lvae_sse_u16(a.data(), ar.data(), b.data(), br.data(), hw.data(), B, out, nullptr));
    b[B - 1] = wdev;
    EXPECT22(lvae_sse_u16(a.data(), ar.data(), b.data(), br.data(), hw.data(), B, nullptr, nullptr));
    hw[0] = 2147483647; hw[1] = 2147483647; ar[0] = br[0] = 2147483647;      // a grid beyond what a launch can index
    EXPECT22(lvae_sse_u16(a.data(), ar.data(), b.data(), br.data(), hw.data(), B, out, nullptr));
}

int main() {
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
        general(B);
        semiplanar(B);
        sse_u16(B);
    }
    EXPECT22(lvae_image_yuv_to_f32(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 8, 0, 0, 0, 0, 0, fdev, 0, 64, 64, nullptr));
    EXPECT22(lvae_image_f32_to_yuv(nullptr, 0, 0, 0, 64, 64, nullptr, 1, 8, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    EXPECT22(lvae_image_yuvsp_to_f32(nullptr, nullptr, nullptr, nullptr, nullptr, 1, 10, 0, 0, 0, 0, 0, fdev, 0, 64, 64, nullptr));
    EXPECT22(lvae_image_f32_to_yuvsp(nullptr, 0, 0, 0, 64, 64, nullptr, 1, 10, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
    EXPECT22(lvae_sse_u16(nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr));
    {                                                                       // the 8-bit entries take BT.601 / BT.709 only
        const uint8_t* y1[1] = {dev};
        uint8_t* yo1[1] = {dev};
        const long yr1[1] = {64}, cr1[1] = {32};
        const int hw1[2] = {8, 8};
        EXPECT22(lvae_image_yuv420_to_f32(y1, y1, y1, yr1, cr1, cr1, hw1, 1, LVAE_YUV_I420, LVAE_YUV_BT2020, LVAE_YUV_LIMITED, LVAE_YUV_BILINEAR,
                                          fdev, 3L * 64 * 64, 64, 64, nullptr));
        EXPECT22(lvae_image_f32_to_yuv420(fdev, 3L * 64 * 64, 64 * 64, 64, 64, 64, hw1, 1, LVAE_YUV_I420, LVAE_YUV_BT2020, LVAE_YUV_LIMITED, yo1, yo1,
                                          yo1, yr1, cr1, cr1, nullptr));
    }
    EXPECT22(lvae_image_yuv420_to_f32(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0, 0, 0, 0, fdev, 0, 64, 64, nullptr));
    EXPECT22(lvae_image_f32_to_yuv420(nullptr, 0, 0, 0, 64, 64, nullptr, 1, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    EXPECT22(lvae_sse_u8(nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr));
    std::printf(fails ? "FAILED %d\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
