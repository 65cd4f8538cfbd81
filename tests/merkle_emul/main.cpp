// The Merkle scheme's lane code (heartbeat_amd/csrc/hb_merkle.hpp) and the
// host chain (hb_merkle_host.hpp) as a plain C++ program, for
// tests/test_merkle_emul.py.  Reads one command per line from the file named
// on the command line and prints one hex token per command ("-" stands for an
// empty byte string in either direction):
//   L key seed n            the n leaf seeds of the chain, by the lane functions
//                           (hb_mk_key, hb_mk_hmac, hb_mk_link) -- and by
//                           mk_host_chain, which must agree
//   H blob index            the leaf hash
//   N left right nchild     the node hash of 0, 1 or 2 children
//   T n blob...             a whole tree: (2 << order) x 32 bytes, empty slots zero
//   O n                     the order (decimal)
//   P n filesz chunksz len  mk_plan_encode of one file: "E<code>" when refused, else
//                           chunk:range:nb:topmask:order:jobs:nodes (decimal)
//   C count                 hb_mk_compress_portable against the lane's
//                           hb_sha256_compress on `count` blocks: 1 if all agree
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hb_merkle_host.hpp"

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

static void words_of(const Bytes &b, u32 w[8]) {
    for (int t = 0; t < 8; ++t)
        w[t] = ((u32)b[4 * t] << 24) | ((u32)b[4 * t + 1] << 16) | ((u32)b[4 * t + 2] << 8) | b[4 * t + 3];
}

static std::string hex_words(const u32 w[8]) {
    unsigned char b[32];
    for (int t = 0; t < 8; ++t)
        for (int k = 0; k < 4; ++k) b[4 * t + k] = (unsigned char)(w[t] >> (24 - 8 * k));
    return hex(b, 32);
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string op;
        ss >> op;
        if (op == "L") {
            std::string k, s;
            unsigned n;
            ss >> k >> s >> n;
            const Bytes key = unhex(k), seed = unhex(s);
            MkFile F;
            memset(&F, 0, sizeof F);
            F.n = n;
            hb_mk_key(key.data(), key.size(), F.key);
            hb_mk_hmac(F.key, seed.data(), seed.size(), F.s1);
            std::string lane;
            u32 cur[8], nx[8];
            for (int t = 0; t < 8; ++t) cur[t] = F.s1[t];
            for (unsigned i = 0; i < n; ++i) {
                lane += hex_words(cur);
                hb_mk_link(F.key, cur, nx);
                for (int t = 0; t < 8; ++t) cur[t] = nx[t];
            }
            Bytes host((size_t)n * 32);
            hbhost::mk_host_chain(F, host.data());
            if (hex(host.data(), host.size()) != lane) {
                fprintf(stderr, "mk_host_chain differs from the lane chain\n");
                return 1;
            }
            std::cout << lane << "\n";
        } else if (op == "H") {
            std::string b;
            u32 index, w[8], h[8];
            ss >> b >> index;
            words_of(unhex(b), w);
            hb_mk_leaf_hash(w, index, h);
            std::cout << hex_words(h) << "\n";
        } else if (op == "N") {
            std::string l, r;
            u32 nchild, lw[8] = {0}, rw[8] = {0}, h[8];
            ss >> l >> r >> nchild;
            if (nchild >= 1) words_of(unhex(l), lw);
            if (nchild >= 2) words_of(unhex(r), rw);
            hb_mk_node_hash(lw, rw, nchild, h);
            std::cout << hex_words(h) << "\n";
        } else if (op == "T") {
            u32 n;
            ss >> n;
            const u32 order = hb_mk_order(n);
            // the buffer's exact size: an index past it is the sanitizer's to find
            std::vector<u32> nodes((size_t)(2u << order) * 8, 0u);
            for (u32 k = 0; k < n; ++k) {
                std::string b;
                ss >> b;
                u32 w[8], h[8];
                words_of(unhex(b), w);
                hb_mk_leaf_hash(w, k, h);
                for (int t = 0; t < 8; ++t) nodes[((size_t)(1u << order) - 1 + k) * 8 + t] = hb_mk_bswap(h[t]);
            }
            for (u32 i = 1; i <= order; ++i)
                for (u32 j = 0; j < (1u << (order - i)); ++j) hb_mk_tree_node(nodes.data(), order, n, i, j);
            std::cout << hex((const unsigned char *)nodes.data(), nodes.size() * 4) << "\n";
        } else if (op == "P") {
            // the descriptor checks and the table entry of one file (mk_plan_encode)
            unsigned long long n, filesz, chunksz, len;
            ss >> n >> filesz >> chunksz >> len;
            static unsigned char byte, nodes[64];
            hb_merkle_encode_desc d;
            memset(&d, 0, sizeof d);
            d.key = d.seed = d.data = &byte;
            d.key_len = d.seed_len = 1;
            d.n = n;
            d.filesz = filesz;
            d.chunksz = chunksz;
            d.len = len;
            d.nodes_out = nodes;
            hbhost::MkPlan P;
            int code = 0;
            std::string err;
            if (!hbhost::mk_plan_encode(&d, 1, P, code, err)) {
                std::cout << "E" << code << "\n";
            } else {
                const MkFile &F = P.files[0];
                std::cout << F.chunk << ":" << (((u64)F.R[1] << 32) | F.R[0]) << ":" << F.nb << ":" << F.topmask << ":"
                          << F.order << ":" << P.jobs << ":" << P.nodes << "\n";
            }
        } else if (op == "O") {
            unsigned long long n;
            ss >> n;
            std::cout << hb_mk_order(n) << "\n";
        } else if (op == "C") {
            unsigned count;
            ss >> count;
            u64 x = 0x9E3779B97F4A7C15ull;
            int same = 1;
            u32 a[8], b[8];
            hb_mk_init(a);
            hb_mk_init(b);
            for (unsigned i = 0; i < count; ++i) {
                u32 W1[16], W2[16];
                for (int t = 0; t < 16; ++t) {
                    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                    W1[t] = W2[t] = (u32)(x >> 16);
                }
                hb_mk_compress_portable(a, W1);
                hb_sha256_compress(b, W2);
                for (int t = 0; t < 8; ++t) same &= a[t] == b[t];
            }
            std::cout << same << "\n";
        } else if (!op.empty()) {
            fprintf(stderr, "unknown command %s\n", op.c_str());
            return 2;
        }
    }
    return 0;
}
