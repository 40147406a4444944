// Test-only: the marshalling of gs_renderer_edit_select_surface's rectangle (csrc/gs_params.h: pick_select_of) compiled for the HOST, so that
// tests/test_pick_model.py can hold the clipping to the numpy twin on a box without a GPU -- the extremes of int32 included.  Never part of the shipped library.
#include "../unitygaussiansplatting_amd/csrc/gs_params.h"

extern "C" {
// out: x0, y0, w, h, stride, tag, subtract
void ph_select_of(int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint32_t width, uint32_t height, uint32_t tag, int32_t subtract, uint32_t out[7]) {
    const gsm::PickSelect S = gs::pick_select_of(x0, y0, x1, y1, width, height, tag, subtract);
    out[0] = S.x0; out[1] = S.y0; out[2] = S.w; out[3] = S.h; out[4] = S.stride; out[5] = S.tag; out[6] = S.subtract;
}
}

#ifdef PICK_HARNESS_MAIN
#include <limits.h>
#include <stdio.h>
int main() {
    const int32_t v[] = { INT_MIN, INT_MIN + 1, -1, 0, 1, 63, 64, 65, 65534, 65535, INT_MAX - 1, INT_MAX };
    unsigned long long checked = 0;
    for (int32_t a : v) for (int32_t b : v) for (int32_t c : v) for (int32_t d : v) {
        if (a > c || b > d) continue;                              // (refused by the entry point before the marshalling)
        const uint32_t widths[] = { 1u, 64u, 65535u };
        for (uint32_t w : widths) {
            uint32_t o[7];
            ph_select_of(a, b, c, d, w, 48u, 7u, 1, o);
            if (o[2] && (o[0] + o[2] > w || o[1] + o[3] > 48u)) { printf("rectangle leaves the target\n"); return 1; }
            if ((o[2] == 0) != (o[3] == 0)) { printf("half-empty rectangle\n"); return 1; }
            ++checked;
        }
    }
    printf("ok %llu\n", checked);
    return 0;
}
#endif
