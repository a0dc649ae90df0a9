// Reads tests/golden/gemm_tile_choices.txt and compares csrc/gemm_plan.cpp's choice for every problem with the recorded one
// (tests/test_gemm_plan.py builds and runs this with the host compiler: no GPU).  A line is a label followed by key=value
// fields:
//   M N K          the problem; leading dimensions are the natural ones (lda = ldw = K, the others N)
//   resid          none | f32 | pair          resid_mod   rows of the residual
//   out            f32 | f16 | f32+f16 | pair
//   stats          1: writes row statistics   ln          ln_groups of a LayerNorm-folded consumer, 0: not one
//   act shared alone unit preset              GemmArgs::act, shared_gpu, alone, unit_rows, tile
//   tile           what gemm_pick_tile returns (-1: no tile / the preset one does not fit), -2: gemm_check refuses
// `--record` prints the file with the tile fields as this build chooses them instead of comparing.
#include "gemm_plan.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>

namespace dlimg {
void throw_error(const char* msg) { throw std::runtime_error(msg); }
}  // namespace dlimg

using namespace dlimg;

static int choice(std::map<std::string, std::string> const& f) {
    auto num = [&](const char* key) { return std::stoi(f.at(key)); };
    // the planner looks at addresses for alignment only; nothing is dereferenced
    alignas(16) static char mem[1];
    half_t* h = reinterpret_cast<half_t*>(mem);
    float* p = reinterpret_cast<float*>(mem);
    k::GemmArgs a;
    a.M = num("M"); a.N = num("N"); a.K = num("K");
    a.A = h; a.W = h; a.lda = a.ldw = a.K; a.bias = p;
    const std::string resid = f.at("resid"), out = f.at("out");
    if (resid == "f32") { a.resid = p; a.ldr = a.N; }
    else if (resid == "pair") { a.resid_h = a.resid_l = h; a.ldrs = a.N; }
    else if (resid != "none") throw std::runtime_error("resid=" + resid);
    a.resid_mod = num("resid_mod");
    if (out == "f32" || out == "f32+f16") { a.out_f32 = p; a.ldc32 = a.N; }
    if (out == "f16" || out == "f32+f16" || out == "pair") { a.out_h = h; a.ldc16 = a.N; }
    if (out == "pair") a.out_l = h;
    if (!a.out_f32 && !a.out_h) throw std::runtime_error("out=" + out);
    if (num("stats")) a.stats_out = p;
    if (num("ln")) { a.ln_stats = p; a.ln_colsum = p; a.ln_groups = num("ln"); a.ln_eps = 1e-6f; }
    a.act = num("act"); a.shared_gpu = num("shared") != 0; a.alone = num("alone") != 0;
    a.unit_rows = num("unit"); a.tile = num("preset");
    if (k::gemm_check(a)) return -2;
    const int tile = k::gemm_pick_tile(a);
    if (tile >= 0 && !k::gemm_tile_fits(a, tile)) throw std::runtime_error("picked a tile that does not fit");
    return tile;
}

int main(int argc, char** argv) {
    const bool record = argc == 3 && !std::strcmp(argv[2], "--record");
    if (argc < 2 || (argc > 2 && !record)) { std::fprintf(stderr, "usage: %s choices.txt [--record]\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    int checked = 0, differ = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') { if (record) std::cout << line << "\n"; continue; }
        std::istringstream words(line);
        std::string label, word, rest;
        std::map<std::string, std::string> f;
        words >> label;
        while (words >> word) {
            const size_t eq = word.find('=');
            if (eq == std::string::npos) { std::printf("malformed: %s\n", line.c_str()); return 1; }
            f[word.substr(0, eq)] = word.substr(eq + 1);
            if (word.compare(0, 5, "tile=")) rest += " " + word;
        }
        int tile;
        try {
            tile = choice(f);
            if (!record && tile != std::stoi(f.at("tile"))) { std::printf("chooses %d: %s\n", tile, line.c_str()); ++differ; }
        } catch (std::exception const& e) { std::printf("%s: %s\n", e.what(), line.c_str()); return 1; }
        if (record) std::cout << label << rest << " tile=" << tile << "\n";
        ++checked;
    }
    if (!record) std::printf("%d problems, %d differ\n", checked, differ);
    return differ ? 1 : 0;
}
