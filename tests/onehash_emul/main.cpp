// The OneHash scheme's lane code (heartbeat_amd/csrc/hb_onehash.hpp) and host
// side (hb_onehash_host.hpp) as a plain C++ program, for
// tests/test_onehash_emul.py.  Reads one command per line from the file named
// on the command line and prints one token per command ("-" stands for an
// empty byte string in either direction):
//   F path                  load a file into a heap buffer of its exact size
//   R block seed            the response of (block, seed) over the loaded file: the plan
//                           rule, the bounds check and the segment hash, with the
//                           file at each of four alignments and through the gather
//                           (oh_gather_job, a slot of exactly chunk bytes), which
//                           must all agree; "E" when the plan leaves the file
//   P size block            the plan: off0:len0:off1:len1 (decimal)
//   L s0 secret n           the n seeds of the chain, by hb_oh_secret / hb_oh_link
//                           where the secret fits (<= 87 bytes) and by
//                           oh_host_chain, which must agree
//   G len num block secret_len null   oh_plan_generate of one file (num blocks, all
//                           `block`); null: 0 none, 1 s0, 2 secret, 3 data, 4 blocks,
//                           5 the outputs.  "E<code>" when refused, else
//                           jobs:flags of the table entry
//   M len file block seed_len null   oh_plan_meet of one job over two files of len
//                           bytes; null: 0 none, 1 files, 2 jobs, 3 the output,
//                           4 the files' data.  "E<code>" or the sorted order
//   U jobs                  oh_upload_max (decimal)
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hb_onehash_host.hpp"

typedef std::vector<unsigned char> Bytes;

static Bytes unhex(const std::string &s) {
    Bytes out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((unsigned char)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

static std::string hex(const unsigned char *p, size_t n) {
    static const char *d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        s.push_back(d[p[i] >> 4]);
        s.push_back(d[p[i] & 15]);
    }
    return s.empty() ? "-" : s;
}

static std::string hex_words(const u32 w[8]) {
    unsigned char b[32];
    hbhost::oh_bytes(w, b);
    return hex(b, 32);
}

// a heap copy of exactly n bytes (n = 0: one byte, never read)
static unsigned char *exact(const unsigned char *src, size_t n) {
    unsigned char *p = (unsigned char *)malloc(n ? n : 1);
    if (n) memcpy(p, src, n);
    return p;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    Bytes file;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string op;
        ss >> op;
        if (op == "F") {
            std::string path;
            ss >> path;
            std::ifstream f(path, std::ios::binary);
            file.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
            std::cout << file.size() << "\n";
        } else if (op == "R") {
            unsigned long long block;
            std::string sd;
            ss >> block >> sd;
            const Bytes seed_v = unhex(sd);
            const u64 fs = file.size();
            if (!(block < fs)) {
                std::cout << "E\n";
                continue;
            }
            const HbOhPlan P = hb_oh_plan(fs, block);
            if (!hb_oh_plan_inside(P, fs)) {
                std::cout << "E\n";
                continue;
            }
            unsigned char *seed = exact(seed_v.data(), seed_v.size());
            std::string first;
            for (size_t k = 0; k < 4; ++k) {
                // the file's last byte is the allocation's last: a load past it is the sanitizer's to find
                unsigned char *buf = (unsigned char *)malloc(fs + k ? fs + k : 1);
                if (fs) memcpy(buf + k, file.data(), fs);
                u32 d[8];
                hb_oh_hash(buf + k, fs, P, seed, seed_v.size(), d);
                free(buf);
                if (k == 0) first = hex_words(d);
                else if (hex_words(d) != first) {
                    fprintf(stderr, "alignment %zu changes the response\n", k);
                    return 1;
                }
            }
            const u64 c = hb_oh_chunk(fs);
            unsigned char *slot = (unsigned char *)malloc(c ? c : 1);
            if (!hbhost::oh_gather_job(file.data(), fs, block, slot)) return 1;
            HbOhPlan Q = P;
            Q.off0 = 0;
            Q.off1 = P.len0;
            u32 d[8];
            if (!hb_oh_plan_inside(Q, c)) return 1;
            hb_oh_hash(slot, c, Q, seed, seed_v.size(), d);
            free(slot);
            free(seed);
            if (hex_words(d) != first) {
                fprintf(stderr, "the gathered segments hash differently\n");
                return 1;
            }
            std::cout << first << "\n";
        } else if (op == "P") {
            unsigned long long size, block;
            ss >> size >> block;
            const HbOhPlan P = hb_oh_plan(size, block);
            std::cout << P.off0 << ":" << P.len0 << ":" << P.off1 << ":" << P.len1 << "\n";
        } else if (op == "L") {
            std::string s0, sec;
            unsigned n;
            ss >> s0 >> sec >> n;
            const Bytes s0b = unhex(s0), secret_v = unhex(sec);
            unsigned char *secret = exact(secret_v.data(), secret_v.size());
            OhFile F;
            memset(&F, 0, sizeof F);
            F.n = n;
            hbhost::oh_words(s0b.data(), F.s0);
            std::string lane;
            const bool fits = hb_oh_secret(secret, secret_v.size(), F.secret);
            if ((secret_v.size() <= HB_ONEHASH_MAX_SECRET) != fits) return 1;
            if (fits) {
                u32 cur[8], nx[8];
                for (int t = 0; t < 8; ++t) cur[t] = F.s0[t];
                for (unsigned i = 0; i < n; ++i) {
                    lane += hex_words(cur);
                    hb_oh_link(F.secret, cur, nx);
                    for (int t = 0; t < 8; ++t) cur[t] = nx[t];
                }
            } else {
                F.flags |= HB_OH_HOST_CHAIN;
            }
            unsigned char *host = (unsigned char *)malloc(n ? (size_t)n * 32 : 1);
            hbhost::oh_host_chain(F, secret, secret_v.size(), host);
            std::string hs = n ? hex(host, (size_t)n * 32) : "";
            if (fits) {
                // and the generic link, as a file with a long secret takes it
                F.flags |= HB_OH_HOST_CHAIN;
                hbhost::oh_host_chain(F, secret, secret_v.size(), host);
                if ((n ? hex(host, (size_t)n * 32) : "") != hs || hs != lane) {
                    fprintf(stderr, "the chains differ\n");
                    return 1;
                }
            }
            free(host);
            free(secret);
            std::cout << (hs.empty() ? "-" : hs) << "\n";
        } else if (op == "G") {
            unsigned long long len, num, block, secret_len;
            int null;
            ss >> len >> num >> block >> secret_len >> null;
            static unsigned char byte[256], s0[32], outs[64];
            std::vector<uint64_t> blocks((size_t)(num < 1024 ? num : 1024), block);   // the checks stop before a larger num is read
            hb_onehash_gen_desc d;
            memset(&d, 0, sizeof d);
            d.data = null == 3 ? nullptr : byte;   // never read by the checks
            d.len = len;
            d.s0 = null == 1 ? nullptr : s0;
            d.secret = null == 2 ? nullptr : byte;
            d.secret_len = secret_len;
            d.num = num;
            d.blocks = null == 4 ? nullptr : blocks.data();
            hbhost::OhPlan P;
            int code = 0;
            std::string err;
            if (!hbhost::oh_plan_generate(&d, 1, null == 5 ? nullptr : outs, null == 5 ? nullptr : outs, P, code, err))
                std::cout << "E" << code << "\n";
            else
                std::cout << P.jobs << ":" << P.files[0].flags << "\n";
        } else if (op == "M") {
            unsigned long long len, file_i, block, seed_len;
            int null;
            ss >> len >> file_i >> block >> seed_len >> null;
            static unsigned char byte, outs[96];
            hb_onehash_file files[2] = {{null == 4 ? nullptr : &byte, len}, {null == 4 ? nullptr : &byte, len}};
            hb_onehash_job jobs[3];
            memset(jobs, 0, sizeof jobs);
            jobs[0].file = 1;
            jobs[1].file = file_i;
            jobs[1].block = block;
            jobs[1].seed_len = seed_len;
            jobs[2].file = 0;
            hbhost::OhPlan P;
            std::vector<size_t> order;
            int code = 0;
            std::string err;
            if (!hbhost::oh_plan_meet(null == 1 ? nullptr : files, 2, null == 2 ? nullptr : jobs, 3,
                                      null == 3 ? nullptr : outs, P, order, code, err)) {
                std::cout << "E" << code << "\n";
            } else {
                std::cout << order[0] << order[1] << order[2] << ":" << P.files[0].job0 << P.files[1].job0 << "\n";
            }
        } else if (op == "U") {
            unsigned long long jobs;
            ss >> jobs;
            std::cout << hbhost::oh_upload_max(jobs) << "\n";
        } else if (!op.empty()) {
            fprintf(stderr, "unknown command %s\n", op.c_str());
            return 2;
        }
    }
    return 0;
}
