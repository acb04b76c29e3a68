// TEST INFRASTRUCTURE ONLY.  A stand-alone program around oracle/restate.cpp's ref_render for frames that have no horizontal or no
// vertical neighbour (1 x 1, 33 x 1, 1 x 33): the records are a heap block of exactly width * height records, so that a read of the
// record before or behind them - which is what the reference's own indexing does there - is an error under AddressSanitizer.
// Built and run by tests/test_shading_model.py with -fsanitize=address and any metric's macros.
#include "restate.cpp"

#include <cstdio>
#include <cstdlib>

int main() {
    const int bgw = 5, bgh = 3, levels = 1, sizes[3][2] = {{1, 1}, {33, 1}, {1, 33}};
    unsigned state = 12345u;
    auto next = [&]() { state = state * 1664525u + 1013904223u; return state >> 8; };
    uint8_t* sky1 = (uint8_t*)std::malloc((size_t)levels * bgw * bgh * 4);
    uint8_t* sky2 = (uint8_t*)std::malloc((size_t)levels * bgw * bgh * 4);
    for (int i = 0; i < levels * bgw * bgh * 4; i++) { sky1[i] = (uint8_t)next(); sky2[i] = (uint8_t)next(); }
    char features[48] = {0};   // every feature off: plain shading
    float cfg[16] = {0};
    int frames = 0;
    for (auto& size : sizes) {
        const int w = size[0], h = size[1], n = w * h;
        render_data* records = (render_data*)std::malloc(sizeof(render_data) * n);
        float* out = (float*)std::malloc(sizeof(float) * 4 * n);
        for (int i = 0; i < n; i++) {
            std::memset(&records[i], 0, sizeof(render_data));
            records[i].sx = i % w;
            records[i].sy = i / w;
            records[i].terminated = 1;
            records[i].side = i % 2;
            records[i].tex_x = (next() % 100000) / 100000.f;
            records[i].tex_y = (next() % 100000) / 100000.f;
        }
        for (int max_probes : {1, 8}) {
            ref_render(records, &n, n, out, sky1, sky2, bgw, bgh, levels, w, h, max_probes, cfg, features, 1);
            for (int i = 0; i < 4 * n; i++)
                if (!(out[i] >= 0.f && out[i] <= 1.f)) { std::printf("pixel %d of %d x %d is %g\n", i / 4, w, h, out[i]); return 1; }
        }
        std::free(records);
        std::free(out);
        frames++;
    }
    std::free(sky1);
    std::free(sky2);
    std::printf("%d frames shaded\n", frames);
    return 0;
}
