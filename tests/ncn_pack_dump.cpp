// TEST INFRASTRUCTURE: pack_conv4d_planes of csrc/host_pack.h as a stand-alone program (its own main; built against the HIP
// stand-in of tests/hipemu by tests/test_ncn_mode_host.py).  Reads k, co, ci, nh, br and the stored weight from argv[1] (int32 x 5,
// then float32 [k][co][ci][k][k][k]), writes the exponents (int32 x co) and the fp16 stream (uint16) to argv[2].
#include "../patch2pix_amd/csrc/host_pack.h"
#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int hdr[5];
    if (fread(hdr, 4, 5, f) != 5) return 4;
    const int k = hdr[0], co = hdr[1], ci = hdr[2], nh = hdr[3], br = hdr[4];
    std::vector<float> w((size_t)k * k * k * k * co * ci);
    if (fread(w.data(), 4, w.size(), f) != w.size()) return 5;
    fclose(f);
    std::vector<uint16_t> out(p2p::conv4d_planes_halfs(k, nh), 0xffff);
    std::vector<int> texp(co, 12345);
    p2p::pack_conv4d_planes(w.data(), k, co, ci, nh, br, out.data(), texp.data());
    f = fopen(argv[2], "wb");
    if (!f) return 6;
    fwrite(texp.data(), 4, texp.size(), f);
    fwrite(out.data(), 2, out.size(), f);
    fclose(f);
    printf("ncn_pack_dump: ok %zu\n", out.size());
    return 0;
}
