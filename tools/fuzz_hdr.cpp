// Mutation fuzzer for the Radiance .hdr decoder of renderer-rs_amd/host/image_decode.hpp, meant for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/fuzz_hdr tools/fuzz_hdr.cpp
//   /tmp/fuzz_hdr <iterations per seed>
// The seeds are built here: flat, new-style RLE and old-style RLE files, one of them with EXPOSURE lines, one 300 wide.  Every mutant must end in an
// image of the extent its header declares (and then goes through hdr_to_float) or in an ImageError; the sanitizers catch anything else.  A mutant whose
// header declares more than 2^22 texels must not decode from these few bytes unless its lines are runs: the peak of rgbe.size() is printed.
#include <cstdio>
#include <cstdlib>
#include <string>
#include "../renderer-rs_amd/host/image_decode.hpp"

using Bytes = std::vector<uint8_t>;

static Bytes file(const std::string& header, const Bytes& body) {
    Bytes f(header.begin(), header.end());
    f.insert(f.end(), body.begin(), body.end());
    return f;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s iterations\n", argv[0]); return 2; }
    const long iters = atol(argv[1]);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    std::vector<Bytes> seeds;
    const std::string head = "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n";
    seeds.push_back(file(head + "-Y 2 +X 3\n", Bytes{1, 2, 3, 128, 4, 5, 6, 129, 7, 8, 9, 130, 10, 11, 12, 0, 13, 14, 15, 255, 16, 17, 18, 1}));                 // flat
    seeds.push_back(file(head + "-Y 2 +X 8\n", Bytes{2, 2, 0, 8, 133, 10, 129, 20, 2, 30, 31, 8, 1, 2, 3, 4, 5, 6, 7, 8, 136, 7, 136, 128,
                                                     2, 2, 0, 8, 3, 9, 8, 7, 133, 0, 132, 255, 132, 1, 8, 0, 1, 1, 1, 2, 2, 0, 128, 1, 0, 135, 130}));        // new-style RLE
    seeds.push_back(file("#?RGBE\nEXPOSURE=2.0\nEXPOSURE= 0.25\n\n-Y 1 +X 9\n",
                         Bytes{50, 60, 70, 128, 1, 1, 1, 2, 1, 1, 1, 0, 1, 2, 3, 130, 1, 1, 1, 3, 2, 2, 200, 9, 255, 255, 255, 255}));                            // old-style RLE
    {   // 300 x 2: long runs and long literals
        Bytes b;
        for (int y = 0; y < 2; y++) {
            b.insert(b.end(), {2, 2, 1, 44});
            for (int c = 0; c < 4; c++) {
                b.insert(b.end(), {255, (uint8_t)(c + y), 128});
                for (int k = 0; k < 128; k++) b.push_back((uint8_t)(k * 3 + c));
                b.insert(b.end(), {(uint8_t)(128 + 45), 9});
            }
        }
        seeds.push_back(file(head + "-Y 2 +X 300\n", b));
    }
    long total = 0;
    for (size_t a = 0; a < seeds.size(); a++) {
        const Bytes& base = seeds[a];
        { auto img = mirhi::resources::decode_hdr(base.data(), base.size()); if (img.rgbe.size() != (size_t)img.width * img.height * 4) { fprintf(stderr, "seed %zu does not decode\n", a); return 1; } }
        long ok = 0, refused = 0; size_t peak = 0;
        for (long i = 0; i < iters; i++, total++) {
            Bytes m = base;
            const int kind = (int)(rnd() % 6);
            if (kind == 0) m.resize(rnd() % m.size());                                        // truncate
            else if (kind == 1) for (int k = 0; k < 1 + (int)(rnd() % 8); k++) m[rnd() % m.size()] ^= (uint8_t)(1u << (rnd() % 8));
            else if (kind == 2) for (int k = 0; k < 1 + (int)(rnd() % 4); k++) m[rnd() % m.size()] = (uint8_t)rnd();
            else if (kind == 3) { size_t at = rnd() % m.size(), n = rnd() % 64; for (size_t k = 0; k < n && at + k < m.size(); k++) m[at + k] = (uint8_t)(rnd() % 3 ? 0xFF : rnd()); }
            else if (kind == 4) {                                                            // a digit of the resolution line becomes another digit, or one is inserted
                std::vector<size_t> digits;
                for (size_t k = 0; k + 1 < m.size() && k < 80; k++) if (m[k] >= '0' && m[k] <= '9') digits.push_back(k);
                if (!digits.empty()) {
                    const size_t at = digits[rnd() % digits.size()];
                    if (rnd() % 2) m[at] = (uint8_t)('0' + rnd() % 10); else m.insert(m.begin() + (long)at, (uint8_t)('0' + rnd() % 10));
                }
            } else { size_t at = rnd() % m.size(), n = 1 + rnd() % 16; Bytes ins(n); for (auto& v : ins) v = (uint8_t)(rnd() % 4 ? rnd() % 4 : rnd()); m.insert(m.begin() + (long)at, ins.begin(), ins.end()); }
            try {
                auto img = mirhi::resources::decode_hdr(m.data(), m.size());
                if (img.rgbe.size() != (size_t)img.width * img.height * 4 || img.width == 0 || img.height == 0) { fprintf(stderr, "seed %zu mutant %ld: extent and size disagree\n", a, i); return 1; }
                if (img.rgbe.size() > peak) peak = img.rgbe.size();
                if (img.rgbe.size() <= (1u << 22)) { std::vector<float> f(img.rgbe.size()); mirhi::resources::hdr_to_float(img.rgbe.data(), img.rgbe.size() / 4, f.data()); }
                ok++;
            } catch (const mirhi::resources::ImageError&) { refused++; }
        }
        printf("seed %zu (%zu bytes): %ld mutants decoded, %ld refused, largest decoded image %zu bytes\n", a, base.size(), ok, refused, peak);
    }
    printf("%ld mutants, no finding\n", total);
    return 0;
}
