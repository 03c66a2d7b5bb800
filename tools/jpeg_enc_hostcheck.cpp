// Stand-alone host check of the JPEG entropy ENCODER (csrc/pam_jpeg_encode.hpp, header-only, no HIP).  DIR holds the shared matrix as
// tests/jpeg_enc_ref.write_coef_files writes it: TAG.coef (width, height, h_samp, v_samp, quality as int32, then int16 coefficients)
// and TAG.jpg (Pillow's file from the same pixels).  Every case is encoded from a heap block of exactly its coefficients into heap
// blocks of exactly the bound, of exactly the file's size and of every smaller capacity (4 096 evenly spread ones for a large file),
// so a read or a store outside either is an AddressSanitizer report; then seeded hostile buffers: random coefficients of the full
// int16 range, of the codable range and sparse ones, random sizes, samplings, qualities, tables and capacities.  Build and run:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_enc_hostcheck.cpp -o jpeg_enc_hostcheck
//   python -c "import sys; sys.path.insert(0, 'tests'); import jpeg_enc_ref as E; E.write_coef_files(sys.argv[1])" DIR
//   ./jpeg_enc_hostcheck DIR [hostile-buffers]
// Exit status 0 and a summary line when every file equalled Pillow's and every call returned PAM_OK or PAM_E_ARG.
#include <dirent.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../part-aware_measurement_for_3d_pose_estimation_and_tracking_amd/csrc/pam_jpeg_encode.hpp"

static long n_ok = 0, n_arg = 0, n_bad = 0;

static std::vector<uint8_t> slurp(const std::string& name) {
    std::vector<uint8_t> bytes;
    FILE* f = fopen(name.c_str(), "rb");
    if (!f) return bytes;
    uint8_t chunk[65536];
    for (size_t got; (got = fread(chunk, 1, sizeof(chunk), f)) > 0;) bytes.insert(bytes.end(), chunk, chunk + got);
    fclose(f);
    return bytes;
}

// one call with the coefficients and the output each in a fresh heap block of exactly their size -> the file, empty unless PAM_OK
static std::vector<uint8_t> one(const int16_t* src, size_t words, const PamJpegEncodeParams& p, size_t cap) {
    int16_t* coef = (int16_t*)malloc(words ? words * sizeof(int16_t) : 1);
    memcpy(coef, src, words * sizeof(int16_t));
    uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
    size_t n = 0;
    const int rc = pamjpegenc::encode(coef, words, &p, out, cap, &n);
    std::vector<uint8_t> file;
    if (rc == PAM_OK) {
        ++n_ok;
        if (n > cap) ++n_bad;
        else file.assign(out, out + n);
    } else if (rc == PAM_E_ARG) {
        ++n_arg;
    } else {
        ++n_bad;
    }
    free(out);
    free(coef);
    return file;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s DIR [hostile-buffers]\n", argv[0]);
        return 2;
    }
    const int n_hostile = argc > 2 ? atoi(argv[2]) : 2000;
    std::vector<std::string> names;
    DIR* dir = opendir(argv[1]);
    if (!dir) {
        perror(argv[1]);
        return 2;
    }
    while (dirent* e = readdir(dir)) {
        const std::string n = e->d_name;
        if (n.size() > 5 && n.substr(n.size() - 5) == ".coef") names.push_back(std::string(argv[1]) + "/" + n.substr(0, n.size() - 5));
    }
    closedir(dir);
    std::sort(names.begin(), names.end());
    long n_files = 0, n_equal = 0, n_short_refused = 0;
    for (const std::string& name : names) {
        const std::vector<uint8_t> raw = slurp(name + ".coef"), want = slurp(name + ".jpg");
        if (raw.size() < 20 || want.empty()) continue;
        int32_t head[5];
        memcpy(head, raw.data(), sizeof(head));
        const size_t words = (raw.size() - 20) / 2;
        std::vector<int16_t> coef(words);
        memcpy(coef.data(), raw.data() + 20, words * 2);
        PamJpegEncodeParams p;
        memset(&p, 0, sizeof(p));
        p.width = head[0]; p.height = head[1]; p.h_samp = head[2]; p.v_samp = head[3]; p.quality = head[4];
        size_t bound = 0;
        if (pamjpegenc::encode_bound(p.width, p.height, p.h_samp, p.v_samp, &bound) != PAM_OK) { ++n_bad; continue; }
        ++n_files;
        if (one(coef.data(), words, p, bound) == want && one(coef.data(), words, p, want.size()) == want) ++n_equal;
        const size_t step = std::max<size_t>(1, want.size() / 4096);
        for (size_t cap = 0; cap < want.size(); cap += step) {
            const long before = n_arg;
            one(coef.data(), words, p, cap);
            n_short_refused += n_arg - before;
        }
        one(coef.data(), words - 1, p, bound);                           // one word short of the layout
    }
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&rng]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng >> 16; };
    static const int samp[6][2] = {{1, 1}, {2, 1}, {2, 2}, {1, 2}, {4, 1}, {0, 0}};
    for (int k = 0; k < n_hostile; ++k) {
        PamJpegEncodeParams p;
        memset(&p, 0, sizeof(p));
        p.width = (int)(next() % 70) - 1; p.height = (int)(next() % 70) - 1;
        const int* s = samp[next() % (k % 8 ? 3 : 6)];
        p.h_samp = s[0]; p.v_samp = s[1];
        p.quality = (int)(next() % 103) - 1;
        for (int t = 0; t < 2; ++t)
            for (int i = 0; i < 64; ++i) p.quant[t][i] = (uint16_t)(k % 16 ? 1 + next() % 255 : next() % 300);
        size_t bound = 0;
        const bool sized = pamjpegenc::encode_bound(p.width, p.height, p.h_samp, p.v_samp, &bound) == PAM_OK;
        size_t words = 64;
        if (sized) {
            const size_t mw = (p.width + 8 * p.h_samp - 1) / (8 * p.h_samp), mh = (p.height + 8 * p.v_samp - 1) / (8 * p.v_samp);
            words = 64 * mw * mh * (p.h_samp * p.v_samp + 2);
            if (k % 32 == 31) words -= 1 + next() % 64;
        }
        std::vector<int16_t> coef(words);
        const int kind = k % 3;                                           // full int16 range / the codable range / sparse
        for (size_t i = 0; i < words; ++i)
            coef[i] = kind == 0 ? (int16_t)(next() & 0xFFFF) : kind == 1 ? (int16_t)((int)(next() % 2047) - 1023) : (next() % 8 ? 0 : (int16_t)((int)(next() % 511) - 255));
        const size_t cap = k % 4 == 3 ? next() % (bound + 1) : bound;
        const std::vector<uint8_t> file = one(coef.data(), words, p, sized ? cap : 4096);
        if (!file.empty() && (file.size() < 625 || file[0] != 0xFF || file[1] != 0xD8 || file[file.size() - 2] != 0xFF || file.back() != 0xD9)) ++n_bad;
    }
    printf("jpeg_enc_hostcheck: %ld cases (%ld equal to Pillow's file at the bound and at the file's size), %ld short capacities refused, "
           "%d hostile buffers; calls: %ld PAM_OK, %ld PAM_E_ARG, %ld other\n", n_files, n_equal, n_short_refused, n_hostile, n_ok, n_arg, n_bad);
    return (n_bad || n_equal != n_files || n_files == 0) ? 1 : 0;
}
