// The OneHash draw's lane code (heartbeat_amd/csrc/hb_onehash_draw.hpp) and
// the host checks of its two entry points (hb_onehash_host.hpp) as a plain C++
// program, for tests/test_onehash_draw_emul.py.  Reads one command per line
// from the file named on the command line and prints one token per command:
//   D len num key           key: the key words in hex, comma-separated.  Seeds a heap
//                           state of exactly 624 words from a heap key of exactly its
//                           length, draws num positions into a heap array of exactly
//                           num; prints the positions (decimal, comma-separated, "-"
//                           for none), ":" and the 625 state words (8 hex digits each)
//   C len key_words num null   oh_plan_draw of two files, a good one and this one;
//                           null: 0 none, 1 the key, 2 blocks_out.  "E<code>:<0|1>"
//                           when refused (1: the message names file 1), else
//                           jobs:key words in all:states
//   X len key_words num secret_len null   oh_plan_generate_drawn of the same two files;
//                           null: 0 none, 1 the key, 2 blocks_out, 3 s0, 4 secret,
//                           5 data, 6 the outputs.  As C, then ":" and file 1's flags
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hb_onehash_host.hpp"

static std::string refused(int code, const std::string &err) {
    return "E" + std::to_string(code) + ":" + (err.find("file 1: ") != std::string::npos ? "1" : "0");
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    static uint32_t good_key[2] = {1, 2}, key_buf[2048];
    static uint64_t blocks_buf[8];
    static uint32_t state_buf[HB_MT_STATE_WORDS];
    static unsigned char byte[256], s0[32], outs[64];
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string op;
        ss >> op;
        if (op == "D") {
            unsigned long long len, num;
            std::string ks;
            ss >> len >> num >> ks;
            std::vector<u32> kv;
            std::istringstream ks2(ks);
            std::string w;
            while (std::getline(ks2, w, ',')) kv.push_back((u32)strtoul(w.c_str(), nullptr, 16));
            u32 *key = (u32 *)malloc(kv.size() * 4);
            memcpy(key, kv.data(), kv.size() * 4);
            u32 *mt = (u32 *)malloc(HB_MT_N * 4);
            u64 *out = (u64 *)malloc(num ? num * 8 : 1);
            hb_mt_seed(mt, key, kv.size());
            const u32 index = hb_mt_draw_serial(mt, len, num, out);
            std::string s;
            for (u64 k = 0; k < num; ++k) s += (k ? "," : "") + std::to_string(out[k]);
            if (!num) s = "-";
            s += ":";
            char hex[16];
            for (u32 i = 0; i < HB_MT_N; ++i) {
                snprintf(hex, sizeof hex, "%08x", mt[i]);
                s += hex;
            }
            snprintf(hex, sizeof hex, "%08x", index);
            s += hex;
            free(out);
            free(mt);
            free(key);
            std::cout << s << "\n";
        } else if (op == "C") {
            unsigned long long len, key_words, num;
            int null;
            ss >> len >> key_words >> num >> null;
            hb_onehash_draw_desc d[2];
            memset(d, 0, sizeof d);
            d[0].len = 10;
            d[0].key = good_key;
            d[0].key_words = 2;
            d[0].num = 3;
            d[0].blocks_out = blocks_buf;
            d[1].len = len;
            d[1].key = null == 1 ? nullptr : key_buf;
            d[1].key_words = key_words;
            d[1].num = num;
            d[1].blocks_out = null == 2 ? nullptr : blocks_buf;   // never written by the checks
            d[1].state_out = state_buf;
            hbhost::OhDrawPlan D;
            int code = 0;
            std::string err;
            if (!hbhost::oh_plan_draw(d, 2, D, code, err)) {
                if (!D.draws.empty() || !D.keys.empty()) return 1;   // nothing planned
                std::cout << refused(code, err) << "\n";
            } else {
                if (D.draws.size() != 2 || D.draws[1].key0 != 2 || D.draws[1].job0 != 3) return 1;
                std::cout << D.jobs << ":" << D.keys.size() << ":" << (D.states ? 1 : 0) << "\n";
            }
        } else if (op == "X") {
            unsigned long long len, key_words, num, secret_len;
            int null;
            ss >> len >> key_words >> num >> secret_len >> null;
            hb_onehash_drawn_desc d[2];
            memset(d, 0, sizeof d);
            for (int i = 0; i < 2; ++i) {
                d[i].data = byte;   // never read by the checks
                d[i].len = 10;
                d[i].s0 = s0;
                d[i].secret = byte;
                d[i].secret_len = 3;
                d[i].num = 3;
                d[i].key = good_key;
                d[i].key_words = 2;
                d[i].blocks_out = blocks_buf;
            }
            d[1].len = len;
            d[1].num = num;
            d[1].secret_len = secret_len;
            d[1].key = null == 1 ? nullptr : key_buf;
            d[1].key_words = key_words;
            if (null == 2) d[1].blocks_out = nullptr;
            if (null == 3) d[1].s0 = nullptr;
            if (null == 4) d[1].secret = nullptr;
            if (null == 5) d[1].data = nullptr;
            hbhost::OhPlan P;
            hbhost::OhDrawPlan D;
            int code = 0;
            std::string err;
            if (!hbhost::oh_plan_generate_drawn(d, 2, null == 6 ? nullptr : outs, null == 6 ? nullptr : outs, P, D, code,
                                                err)) {
                if (!D.draws.empty() || !D.keys.empty()) return 1;
                std::cout << refused(code, err) << "\n";
            } else {
                if (D.draws.size() != 2 || P.files.size() != 2 || P.jobs != D.jobs || P.files[1].job0 != D.draws[1].job0)
                    return 1;
                std::cout << D.jobs << ":" << D.keys.size() << ":" << (D.states ? 1 : 0) << ":" << P.files[1].flags << "\n";
            }
        } else if (!op.empty()) {
            fprintf(stderr, "unknown command %s\n", op.c_str());
            return 2;
        }
    }
    return 0;
}
