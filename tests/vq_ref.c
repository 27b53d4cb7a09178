/* include/gs_vq.h's assignment restated with libm's fmaf: compiled by vq_ref.py with gcc -O2 -ffp-contract=off. */
#include <math.h>
#include <stdint.h>

static float pad(const float* row, int dim, int j) { return j < dim ? row[j] : 0.0f; }

void vq_ref_assign(const float* x, int64_t ldx, int64_t n_rows, int dim, const float* cb, int64_t ldc, int n_codes, float* cc /* (K) work */,
                   int32_t* labels, float* dist)
{
    const int Dp = (dim + 3) / 4 * 4;
    for (int k = 0; k < n_codes; ++k) {
        float acc = 0.0f;
        for (int j = 0; j < Dp; ++j) acc = fmaf(pad(cb + k * ldc, dim, j), pad(cb + k * ldc, dim, j), acc);
        cc[k] = acc;
    }
    for (int64_t n = 0; n < n_rows; ++n) {
        const float* xr = x + n * ldx;
        float xx = 0.0f, best = INFINITY;
        int32_t label = -1;
        for (int j = 0; j < Dp; ++j) xx = fmaf(pad(xr, dim, j), pad(xr, dim, j), xx);
        for (int k = 0; k < n_codes; ++k) {
            float s = cc[k];
            for (int j = 0; j < Dp; ++j) s = fmaf(pad(xr, dim, j), -2.0f * pad(cb + k * ldc, dim, j), s);
            if (isfinite(cc[k]) && s < best) { best = s; label = k; }
        }
        if (!isfinite(xx)) label = -1;
        labels[n] = label;
        dist[n] = label < 0 ? NAN : fmaxf(0.0f, xx + best);
    }
}
