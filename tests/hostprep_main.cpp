// The host-only entry points of csrc/rope_hostprep.cpp as a program of their own, built by tests/test_hostprep_host.py together with
// that file under AddressSanitizer and UBSan: every call gets heap buffers of exactly the size include/rope_s3d.h promises, at the
// edges (strides larger than rows, nothing to merge, a window wider than the image, a capacity one short, ...), and prints one
// line: its name, its return code and the FNV-1a hash of its output bytes.  The test makes the same calls on the shipped library
// through ctypes, from the same inputs — val() below, written out again in Python — and compares the lines.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../include/rope_s3d.h"

static uint32_t val(uint32_t seed, uint32_t i) { return ((i + seed) * 2654435761u) >> 16; }      // 16 bits

// a heap block of exactly n bytes (new[] of the exact size: one byte past it is the sanitizer's)
struct Block {
    size_t n;
    std::unique_ptr<unsigned char[]> p;
    explicit Block(size_t bytes, int fill = 0) : n(bytes), p(new unsigned char[bytes]) { std::memset(p.get(), fill, bytes); }
    template <typename T> T *as() { return reinterpret_cast<T *>(p.get()); }
};

static void report(const std::string &name, long long rc, std::initializer_list<Block *> outs)
{
    uint64_t h = 1469598103934665603ull;
    for (Block *b : outs)
        for (size_t i = 0; i < b->n; i++) h = (h ^ b->p[i]) * 1099511628211ull;
    std::printf("%s rc=%lld fnv=%016llx\n", name.c_str(), rc, (unsigned long long)h);
}

// H rows of W x ch values `stride` bytes apart, the last row as short as its values; value (y, x, c) = f(index)
template <typename T, typename F> static Block image(int H, int W, int ch, size_t stride, F f)
{
    Block b((size_t)(H - 1) * stride + (size_t)W * ch * sizeof(T), 0xAA);
    for (int y = 0; y < H; y++)
        for (int i = 0; i < W * ch; i++) {
            const T v = f((uint32_t)(y * W * ch + i));
            std::memcpy(b.p.get() + (size_t)y * stride + (size_t)i * sizeof(T), &v, sizeof(T));
        }
    return b;
}

// depths in eighths of a metre, every fifth one missing
static double depth_of(uint32_t seed, uint32_t i) { const uint32_t v = val(seed, i); return v % 5 == 0 ? 0.0 : (double)(v % 37) * 0.125; }

static void downsample()
{
    for (int kind = 0; kind < 3; kind++)
        for (int f = 1; f <= 2; f++) {
            const int H = 4, W = 6, ch = kind == 0 ? 3 : 1;
            const size_t elem = kind == 0 ? 1 : (kind == 1 ? 4 : 8), stride = (size_t)W * ch * elem + 16;
            Block src = kind == 0 ? image<uint8_t>(H, W, ch, stride, [](uint32_t i) { return (uint8_t)val(1, i); })
                      : kind == 1 ? image<float>(H, W, ch, stride, [](uint32_t i) { return (float)depth_of(2, i); })
                                  : image<double>(H, W, ch, stride, [](uint32_t i) { return depth_of(3, i); });
            Block dst((size_t)(H / f) * (W / f) * ch * elem);
            const int rc = rope_downsample_even(src.p.get(), H, W, ch, (int64_t)stride, f, kind, dst.p.get());
            report("downsample_even kind=" + std::to_string(kind) + " f=" + std::to_string(f), rc, {&dst});
        }
}

static void synthetic()
{
    // 4x6 -> 2x3: every 2x2 block one colour; link 3's colour is not in the frame, link 4 has none, link 5's is no byte; the
    // pixels of colour 30 (link 2) have no depth
    const int H0 = 4, W0 = 6, f = 2, H = 2, W = 3;
    const int blue[6] = {10, 10, 20, 20, 30, 30};
    const int32_t link_blue[6] = {10, 20, 30, 40, -1, 300};
    auto colour = [&](uint32_t i) -> uint8_t {
        const int c = i % 3, x = (i / 3) % W0, y = i / (3 * W0);
        return c == 0 ? (uint8_t)blue[(y / 2) * W + x / 2] : (uint8_t)val(4, i);
    };
    auto depth = [&](uint32_t i) { return blue[((i / W0) / 2) * W + (i % W0) / 2] == 30 ? 0.0 : 0.5 + 0.125 * (double)(i % 7); };
    Block color = image<uint8_t>(H0, W0, 3, 3 * W0 + 7, colour);
    for (int kind = 1; kind <= 2; kind++)
        for (int want_depth = 0; want_depth < 2; want_depth++) {
            const size_t stride = (size_t)W0 * (kind == 1 ? 4 : 8) + 8;
            Block d = kind == 1 ? image<float>(H0, W0, 1, stride, [&](uint32_t i) { return (float)depth(i); }) : image<double>(H0, W0, 1, stride, depth);
            Block lb(sizeof link_blue), tq((size_t)H * W * 8), look((size_t)H * W * 4), tgt(want_depth ? (size_t)H * W * 8 : 0), flags(8, 0xFF);
            std::memcpy(lb.p.get(), link_blue, sizeof link_blue);
            const int rc = rope_prepare_synthetic(color.p.get(), 3 * W0 + 7, d.p.get(), kind, (int64_t)stride, H0, W0, f, lb.as<int32_t>(), 6, 3,
                                                  tq.as<uint64_t>(), look.as<float>(), want_depth ? tgt.as<double>() : nullptr, flags.p.get());
            report("prepare_synthetic kind=" + std::to_string(kind) + " tgt=" + std::to_string(want_depth), rc, {&tq, &look, &tgt, &flags});
        }
}

static void segmented()
{
    // 6x8 and 3x4 targets: the 8- and 7-wide windows of the body mask reach past the image on one side or on all
    const int shapes[2][2] = {{6, 8}, {3, 4}};
    for (const auto &hw : shapes)
        for (int f = 1; f <= 2; f++)
            for (int K = 0; K <= 3; K += 3) {
                const int H = hw[0], W = hw[1], H0 = H * f, W0 = W * f, kind = f;      // float32 at f = 1, float64 at f = 2
                const size_t stride = (size_t)W0 * (kind == 1 ? 4 : 8) + 24;
                Block d = kind == 1 ? image<float>(H0, W0, 1, stride, [](uint32_t i) { return (float)depth_of(5, i); })
                                    : image<double>(H0, W0, 1, stride, [](uint32_t i) { return depth_of(6, i); });
                Block masks((size_t)H * W * K), link_of((size_t)K * 4), tq((size_t)H * W * 8), look((size_t)H * W * 4), tgt((size_t)H * W * 8), flags(8, 0xFF);
                for (size_t i = 0; i < masks.n; i++) masks.p[i] = (uint8_t)(val(7, (uint32_t)i) % 3 == 0);
                const int32_t lo[3] = {0, -1, 2};
                if (K) std::memcpy(link_of.p.get(), lo, sizeof lo);
                const int rc = rope_prepare_segmented(d.p.get(), kind, (int64_t)stride, H0, W0, f, K ? masks.p.get() : nullptr, K, K ? link_of.as<int32_t>() : nullptr,
                                                      6, 3, tq.as<uint64_t>(), look.as<float>(), tgt.as<double>(), flags.p.get());
                report("prepare_segmented " + std::to_string(H) + "x" + std::to_string(W) + " f=" + std::to_string(f) + " K=" + std::to_string(K), rc,
                       {&tq, &look, &tgt, &flags});
            }
}

static void grids()
{
    Block limits(12 * 8), div(6 * 4);
    const int32_t divisions[6] = {3, 2, 1, 0, 2, -1};                    // 3 x 2 x 1 x 1 x 2 x 1 = 12 rows
    for (int j = 0; j < 12; j++) limits.as<double>()[j] = (j % 2 ? 1.0 : -1.0) * 0.25 * (double)(1 + val(8, (uint32_t)j) % 9);
    std::memcpy(div.p.get(), divisions, sizeof divisions);
    report("lookup_grid count", rope_lookup_grid(limits.as<double>(), div.as<int32_t>(), nullptr, 0), {});
    for (int capacity = 12; capacity >= 11; capacity--) {
        Block out((size_t)capacity * 6 * 8);
        const long long rc = rope_lookup_grid(limits.as<double>(), div.as<int32_t>(), out.as<double>(), capacity);
        report("lookup_grid capacity=" + std::to_string(capacity), rc, {&out});
    }
    for (int links = 2; links <= 6; links++) {
        Block d(6 * 4, 0xFF);
        report("crop_divisions n_pixels=1 links=" + std::to_string(links), rope_crop_divisions(1, links, d.as<int32_t>()), {&d});
    }
    for (int max_size : {3, 4, 25}) {
        int n = -1;
        const int rc0 = rope_hole_thresholds(0.22, 1.0, max_size, nullptr, &n);
        Block T((size_t)(n > 0 ? n : 0) * 4);
        const int rc = rope_hole_thresholds(0.22, 1.0, max_size, T.as<uint32_t>(), &n);
        report("hole_thresholds max_size=" + std::to_string(max_size) + " n=" + std::to_string(n), rc0 * 100 + rc, {&T});
    }
    Block pose(6 * 8), PV(16 * 8);
    for (int j = 0; j < 6; j++) pose.as<double>()[j] = 0.125 * (double)(val(9, (uint32_t)j) % 17) - 1.0;
    report("camera_matrix", rope_camera_matrix(pose.as<double>(), 600.0, 601.5, 320.25, 239.75, 640, 480, 0.05, 100.0, PV.as<double>()), {&PV});
}

static void pack()
{
    const double depth[8] = {std::numeric_limits<double>::quiet_NaN(), -1.5, 0.0, 1.5, 127.99999999999, 128.0, 1.0e300, std::numeric_limits<double>::infinity()};
    for (int with_mask = 0; with_mask < 2; with_mask++) {
        Block d(sizeof depth), mask(8), out(8 * 8, 0xFF);
        std::memcpy(d.p.get(), depth, sizeof depth);
        for (int i = 0; i < 8; i++) mask.p[i] = (uint8_t)val(10, (uint32_t)i);
        const int rc = rope_pack_target(d.as<double>(), with_mask ? mask.p.get() : nullptr, 8, out.as<uint64_t>());
        report("pack_target mask=" + std::to_string(with_mask), rc, {&out});
    }
}

int main()
{
    downsample();
    synthetic();
    segmented();
    grids();
    pack();
    return 0;
}
