// csrc/batch_draw.h on the host, against vectors of the Python definition (clips.batch_draw_host): DESIGN.md "Batch draw".
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I 2023-tifs-istvt_amd/csrc \
//       tools/batch_draw_check.cpp -o batch_draw_check && ./batch_draw_check vectors.bin
//
// vectors.bin (tests/test_batch_draw_cpu.py writes it): int32 words, little endian.  ncases, then per case: B, T, block_ints,
// the status expected, the block before the draw [block_ints], the block after it [block_ints].  Every case runs in a heap
// copy of exactly block_ints ints, so a read or write outside the block is the sanitizer's to report; the draw is run as the
// kernel runs it -- the header check, the videos rows, the clips, then the step -- and the whole block is compared.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "batch_draw.h"

static int draw(int* block, int B, int T, long block_ints) {
    BdPlan p;
    const int refused = bd_check(block, B, T, block_ints, p);
    const uint64_t step = bd_u64(block, BD_STEP);
    if (refused) {
        block[BD_STATUS] = refused;
        return refused;
    }
    for (int v = 0; v < p.V; ++v)
        if (!bd_video_ok(p, block, v)) {
            block[BD_STATUS] = BD_STATUS_VIDEOS;
            return BD_STATUS_VIDEOS;
        }
    for (int b = 0; b < B; ++b) bd_clip(p, block, step, b);
    const uint64_t next = step + 1;
    block[BD_STEP] = (int)(uint32_t)next, block[BD_STEP + 1] = (int)(uint32_t)(next >> 32);
    block[BD_DRAWN] = (int)(uint32_t)step, block[BD_DRAWN + 1] = (int)(uint32_t)(step >> 32);
    block[BD_STATUS] = 0;
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s vectors.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    std::vector<int> words;
    int buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(int), 4096, f)) > 0) words.insert(words.end(), buf, buf + got);
    fclose(f);
    size_t at = 0;
    auto need = [&](size_t n) {
        if (at + n > words.size()) {
            fprintf(stderr, "vectors end early at word %zu\n", at);
            exit(2);
        }
    };
    need(1);
    const int ncases = words[at++];
    long clips = 0, refused = 0;
    for (int c = 0; c < ncases; ++c) {
        need(4);
        const int B = words[at], T = words[at + 1], ints = words[at + 2], want = words[at + 3];
        at += 4;
        if (B < 1 || T < 1 || ints < BD_HEADER_INTS + (long)B * T) {      // what the entry refuses before a launch
            fprintf(stderr, "case %d: bad scalars\n", c);
            return 2;
        }
        need(2 * (size_t)ints);
        int* block = (int*)malloc(sizeof(int) * (size_t)ints);
        memcpy(block, &words[at], sizeof(int) * (size_t)ints);
        const int* after = &words[at + ints];
        at += 2 * (size_t)ints;
        const int status = draw(block, B, T, ints);
        if (status != want) {
            fprintf(stderr, "case %d: status %d, expected %d\n", c, status, want);
            return 1;
        }
        for (int i = 0; i < ints; ++i)
            if (block[i] != after[i]) {
                fprintf(stderr, "case %d: word %d is %d, expected %d\n", c, i, block[i], after[i]);
                return 1;
            }
        free(block);
        if (status) ++refused; else clips += B;
    }
    printf("draw: %d cases, %ld clips, %ld refused\nok\n", ncases, clips, refused);
    return 0;
}
