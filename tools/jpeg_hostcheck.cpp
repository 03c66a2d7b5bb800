// Stand-alone host check of the JPEG entropy pass (csrc/pam_jpeg_entropy.hpp, header-only, no HIP): walks a directory of files and, for
// every file, every truncation of it and a number of seeded single-byte corruptions, runs the probe and the entropy pass on a copy
// of the bytes in a heap block of exactly that size, into a coefficient block of exactly the size the probe states -- so a read or a
// store outside either is an AddressSanitizer report.  Build and run (see tools/README.md):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_hostcheck.cpp -o jpeg_hostcheck
//   ./jpeg_hostcheck DIR [corruptions-per-file]
// Exit status 0 and a summary line when every call returned PAM_OK or PAM_E_ARG.
#include <dirent.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../part-aware_measurement_for_3d_pose_estimation_and_tracking_amd/csrc/pam_jpeg_entropy.hpp"

static long n_ok = 0, n_arg = 0, n_unsupported = 0, n_bad = 0;

// one probe + entropy pass over exactly n bytes (a fresh heap block: nothing readable behind it)
static void one(const uint8_t* src, size_t n) {
    uint8_t* d = (uint8_t*)malloc(n ? n : 1);
    memcpy(d, src, n);
    PamJpegInfo info;
    const int rc = pamjpeg::probe(d, n, &info);
    if (rc != PAM_OK && rc != PAM_E_ARG) ++n_bad;
    if (rc == PAM_OK && info.unsupported) ++n_unsupported;
    if (rc == PAM_OK && !info.unsupported && info.coef_words > 0 && info.coef_words <= (int64_t)1 << 24) {
        int16_t* coef = (int16_t*)malloc((size_t)info.coef_words * sizeof(int16_t));
        const int rc2 = pamjpeg::entropy(d, n, &info, coef, (size_t)info.coef_words);
        if (rc2 == PAM_OK) ++n_ok;
        else if (rc2 == PAM_E_ARG) ++n_arg;
        else ++n_bad;
        free(coef);
    } else if (rc == PAM_E_ARG) {
        ++n_arg;
    }
    free(d);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s DIR [corruptions-per-file]\n", argv[0]);
        return 2;
    }
    const int n_corrupt = argc > 2 ? atoi(argv[2]) : 200;
    std::vector<std::string> names;
    DIR* dir = opendir(argv[1]);
    if (!dir) {
        perror(argv[1]);
        return 2;
    }
    while (dirent* e = readdir(dir))
        if (e->d_name[0] != '.') names.push_back(std::string(argv[1]) + "/" + e->d_name);
    closedir(dir);
    std::sort(names.begin(), names.end());
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    long n_files = 0, n_whole_ok = 0;
    for (const std::string& name : names) {
        FILE* f = fopen(name.c_str(), "rb");
        if (!f) continue;
        std::vector<uint8_t> bytes;
        uint8_t chunk[65536];
        for (size_t got; (got = fread(chunk, 1, sizeof(chunk), f)) > 0;) bytes.insert(bytes.end(), chunk, chunk + got);
        fclose(f);
        ++n_files;
        const long before = n_ok;
        one(bytes.data(), bytes.size());
        n_whole_ok += n_ok - before;
        // every truncation of a small file, 4 096 evenly spread ones of a large file
        const size_t step = std::max<size_t>(1, bytes.size() / 4096);
        for (size_t cut = 0; cut < bytes.size(); cut += step) one(bytes.data(), cut);
        std::vector<uint8_t> bad;
        for (int k = 0; k < n_corrupt && !bytes.empty(); ++k) {
            bad = bytes;
            rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
            bad[(size_t)(rng >> 16) % bad.size()] = (uint8_t)(rng & 255);
            one(bad.data(), bad.size());
        }
    }
    printf("jpeg_hostcheck: %ld files (%ld decoded whole), calls: %ld PAM_OK, %ld PAM_E_ARG, %ld unsupported, %ld other\n", n_files,
           n_whole_ok, n_ok, n_arg, n_unsupported, n_bad);
    return n_bad ? 1 : 0;
}
