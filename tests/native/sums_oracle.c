/* sums_oracle.c -- the CPU statement of the tracker's window sums for the tests
 * of KLT_HIP_FAST (include/klt_hip.h): the oracle's KLTTrackFeatures loop with
 * every window sum -- gxx, gxy, gyy, ex, ey, the residue and the gain/bias
 * moments s1, s2, q1, q2 (both places they are formed) -- taken by one function,
 * wsum, whose order of addition is a process-wide mode.  The oracle itself is
 * included as it stands; track_one and the lighting-insensitive part of
 * sample_windows are restated here with the terms of each sum laid out in the
 * reference's pixel order before they are added.  Everything outside the sums
 * is the oracle's float code.
 *
 *   SEQ    float, the reference's order: equals orc_track bit for bit
 *   WIDE   double accumulation, rounded to float once per sum (the tests' W)
 *   REV, TREE, PERM(seed)   float sums in other orders
 *   mutants, for the sums of the groups in a mask (others stay SEQ):
 *     DROP_LAST   the last pixel is left out
 *     TWICE_FIRST pixel 0 is counted twice
 *     LEAK        the last pixel is counted 64 * PPL - npx more times (the idle
 *                 slots of a wave that gathers PPL pixels per lane; they read
 *                 the last pixel)
 *     DROP_SLOT   pixels 64..127 are left out (one pass of a lane's pixel loop;
 *                 windows over 64 px only)
 */
#include "../../oracle/klt_oracle.c"

enum { SUM_SEQ = 0, SUM_WIDE, SUM_REV, SUM_TREE, SUM_PERM, SUM_DROP_LAST, SUM_TWICE_FIRST, SUM_LEAK,
       SUM_DROP_SLOT };
enum { GRP_G = 1, GRP_E = 2, GRP_RES = 4, GRP_MOM = 8 };

#define SUMS_MAXPX (64 * 64)

static int g_sum_mode = SUM_SEQ, g_sum_seed = 0, g_sum_groups = 15;
static int g_perm[SUMS_MAXPX], g_perm_n = 0, g_perm_seed = -1;

ORC_EXPORT void orc_sums_mode(int mode, int seed, int groups)
{
  g_sum_mode = mode;
  g_sum_seed = seed;
  g_sum_groups = groups;
}

/* pixels per lane of the generic tracker's instance for a window (track.hip, with_instance) */
ORC_EXPORT int orc_sums_ppl(int npx) { return npx <= 64 ? 1 : npx <= 256 ? 4 : 16; }

/* Fisher-Yates from a 64-bit LCG (Knuth's MMIX constants): depends on (seed, n) alone */
static const int *sum_perm(int n)
{
  if (g_perm_n != n || g_perm_seed != g_sum_seed) {
    uint64_t s = 0x9E3779B97F4A7C15ull * (uint64_t)(g_sum_seed + 1) + (uint64_t)n;
    int i;
    for (i = 0; i < n; i++) g_perm[i] = i;
    for (i = n - 1; i > 0; i--) {
      int j, t;
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      j = (int)((s >> 33) % (uint64_t)(i + 1));
      t = g_perm[i];
      g_perm[i] = g_perm[j];
      g_perm[j] = t;
    }
    g_perm_n = n;
    g_perm_seed = g_sum_seed;
  }
  return g_perm;
}

static float sum_tree(const float *t, int n)
{
  int h;
  if (n == 1) return t[0];
  h = (n + 1) / 2;
  return sum_tree(t, h) + sum_tree(t + h, n - h);
}

/* the sum of t[0..n) -- the reference's terms in its pixel order -- by the mode */
static float wsum(const float *t, int n, int group)
{
  int mode = g_sum_mode, q;
  float acc = 0.0f;
  if (mode >= SUM_DROP_LAST && !(g_sum_groups & group)) mode = SUM_SEQ;
  switch (mode) {
  case SUM_WIDE: {
    double d = 0.0;
    for (q = 0; q < n; q++) d += (double)t[q];
    return (float)d;
  }
  case SUM_REV:
    for (q = n - 1; q >= 0; q--) acc += t[q];
    return acc;
  case SUM_TREE:
    return sum_tree(t, n);
  case SUM_PERM: {
    const int *p = sum_perm(n);
    for (q = 0; q < n; q++) acc += t[p[q]];
    return acc;
  }
  case SUM_DROP_LAST:
    for (q = 0; q < n - 1; q++) acc += t[q];
    return acc;
  case SUM_TWICE_FIRST:
    for (q = 0; q < n; q++) acc += t[q];
    return acc + t[0];
  case SUM_LEAK: {
    const int extra = 64 * orc_sums_ppl(n) - n;
    for (q = 0; q < n; q++) acc += t[q];
    for (q = 0; q < extra; q++) acc += t[n - 1];
    return acc;
  }
  case SUM_DROP_SLOT:
    for (q = 0; q < n; q++)
      if (q < 64 || q >= 128) acc += t[q];
    return acc;
  default:
    for (q = 0; q < n; q++) acc += t[q];
    return acc;
  }
}

/* sample_windows, lighting-insensitive part (trackFeatures.c:133-220) */
static void sample_windows_sums(const orc_level *A, const orc_level *B, float x1, float y1, float x2,
                                float y2, int ww, int wh, int li, float *diff, float *sgx, float *sgy)
{
  const int hw = ww / 2, hh = wh / 2, WA = A->w, WB = B->w, npx = ww * wh;
  float ta[SUMS_MAXPX], tb[SUMS_MAXPX];
  int i, j, q;
  if (!li) {
    sample_windows(A, B, x1, y1, x2, y2, ww, wh, 0, diff, sgx, sgy);
    return;
  }
  {
    float s1, s2, q1, q2, m1, m2, alpha, beta;
    q = 0;
    for (j = -hh; j <= hh; j++)
      for (i = -hw; i <= hw; i++, q++) {
        ta[q] = bilerp(x1 + i, y1 + j, A->img, WA);
        tb[q] = bilerp(x2 + i, y2 + j, B->img, WB);
      }
    s1 = wsum(ta, npx, GRP_MOM);
    s2 = wsum(tb, npx, GRP_MOM);
    for (q = 0; q < npx; q++) {
      ta[q] = ta[q] * ta[q];
      tb[q] = tb[q] * tb[q];
    }
    q1 = wsum(ta, npx, GRP_MOM);
    q2 = wsum(tb, npx, GRP_MOM);
    m1 = q1 / (ww * wh);
    m2 = q2 / (ww * wh);
    alpha = (float)sqrt(m1 / m2);
    m1 = s1 / (ww * wh);
    m2 = s2 / (ww * wh);
    beta = m1 - alpha * m2;
    q = 0;
    for (j = -hh; j <= hh; j++)
      for (i = -hw; i <= hw; i++, q++) {
        float a = bilerp(x1 + i, y1 + j, A->img, WA);
        float b = bilerp(x2 + i, y2 + j, B->img, WB);
        diff[q] = a - b * alpha - beta;
      }
  }
  if (sgx) {
    float s1, s2, m1, m2, alpha;
    q = 0;
    for (j = -hh; j <= hh; j++)
      for (i = -hw; i <= hw; i++, q++) {
        ta[q] = bilerp(x1 + i, y1 + j, A->img, WA);
        tb[q] = bilerp(x2 + i, y2 + j, B->img, WB);
      }
    s1 = wsum(ta, npx, GRP_MOM);
    s2 = wsum(tb, npx, GRP_MOM);
    m1 = s1 / (ww * wh);
    m2 = s2 / (ww * wh);
    alpha = (float)sqrt(m1 / m2);
    q = 0;
    for (j = -hh; j <= hh; j++)
      for (i = -hw; i <= hw; i++, q++) {
        float a = bilerp(x1 + i, y1 + j, A->gx, WA);
        float b = bilerp(x2 + i, y2 + j, B->gx, WB);
        sgx[q] = a + b * alpha;
        a = bilerp(x1 + i, y1 + j, A->gy, WA);
        b = bilerp(x2 + i, y2 + j, B->gy, WB);
        sgy[q] = a + b * alpha;
      }
  }
}

/* track_one (_trackFeature, trackFeatures.c:381-486) with its sums through wsum */
static int track_one_sums(float x1, float y1, float *x2, float *y2, const orc_level *A,
                          const orc_level *B, const orc_params *P)
{
  const int ww = P->window_width, wh = P->window_height, npx = ww * wh;
  const int hw = ww / 2, hh = wh / 2, nc = A->w, nr = A->h;
  float diff[SUMS_MAXPX], sgx[SUMS_MAXPX], sgy[SUMS_MAXPX], t[SUMS_MAXPX];
  float gxx, gxy, gyy, ex, ey, dx = 0, dy = 0;
  int it = 0, status = TRACKED, q;

  do {
    if (window_out(x1, y1, hw, hh, nc, nr) || window_out(*x2, *y2, hw, hh, nc, nr)) {
      status = OOB;
      break;
    }
    sample_windows_sums(A, B, x1, y1, *x2, *y2, ww, wh, P->lighting_insensitive, diff, sgx, sgy);
    for (q = 0; q < npx; q++) t[q] = sgx[q] * sgx[q];
    gxx = wsum(t, npx, GRP_G);
    for (q = 0; q < npx; q++) t[q] = sgx[q] * sgy[q];
    gxy = wsum(t, npx, GRP_G);
    for (q = 0; q < npx; q++) t[q] = sgy[q] * sgy[q];
    gyy = wsum(t, npx, GRP_G);
    for (q = 0; q < npx; q++) t[q] = diff[q] * sgx[q];
    ex = wsum(t, npx, GRP_E);
    for (q = 0; q < npx; q++) t[q] = diff[q] * sgy[q];
    ey = wsum(t, npx, GRP_E);
    ex *= P->step_factor;
    ey *= P->step_factor;
    {
      float det = gxx * gyy - gxy * gxy;
      if (det < P->min_determinant) {
        status = SMALL_DET;
        break;
      }
      dx = (gyy * ex - gxy * ey) / det;
      dy = (gxx * ey - gxy * ex) / det;
      status = TRACKED;
    }
    *x2 += dx;
    *y2 += dy;
    it++;
  } while ((fabs(dx) >= P->min_displacement || fabs(dy) >= P->min_displacement) &&
           it < P->max_iterations);

  if (window_out(*x2, *y2, hw, hh, nc, nr)) status = OOB;

  if (status == TRACKED) {
    float s;
    sample_windows_sums(A, B, x1, y1, *x2, *y2, ww, wh, P->lighting_insensitive, diff, NULL, NULL);
    for (q = 0; q < npx; q++) t[q] = (float)fabs(diff[q]);
    s = wsum(t, npx, GRP_RES);
    if (s / (ww * wh) > P->max_residue) status = LARGE_RESIDUE;
  }
  if (status == SMALL_DET) return SMALL_DET;
  if (status == OOB) return OOB;
  if (status == LARGE_RESIDUE) return LARGE_RESIDUE;
  if (it >= P->max_iterations) return MAX_ITERATIONS;
  return TRACKED;
}

/* orc_track (track_impl without the affine check) on track_one_sums */
ORC_EXPORT void orc_track_sums(orc_tracker *t, const uint8_t *img1, const uint8_t *img2, int W, int H,
                               int nfeat, float *fx, float *fy, int *fval)
{
  orc_params *P = &t->P;
  orc_pyr *p1, *p2;
  const float ss = (float)P->subsampling;
  int k, r;

  fix_window(P);
  if (P->window_width * P->window_height > SUMS_MAXPX) {
    fprintf(stderr, "orc_track_sums: window over %d px\n", SUMS_MAXPX);
    abort();
  }
  if (P->sequentialMode && t->last) {
    p1 = t->last;
    if (p1->w[0] != W || p1->h[0] != H) {
      fprintf(stderr, "orc: image size changed in sequential mode\n");
      abort();
    }
  } else {
    p1 = frame_pyramid(P, img1, W, H);
  }
  p2 = frame_pyramid(P, img2, W, H);

  for (k = 0; k < nfeat; k++) {
    float xl, yl, xo, yo;
    int val = TRACKED;
    if (fval[k] < 0) continue;
    xl = fx[k];
    yl = fy[k];
    for (r = P->nPyramidLevels - 1; r >= 0; r--) {
      xl /= ss;
      yl /= ss;
    }
    xo = xl;
    yo = yl;
    for (r = P->nPyramidLevels - 1; r >= 0; r--) {
      orc_level A = {p1->img[r], p1->gx[r], p1->gy[r], p1->w[r], p1->h[r]};
      orc_level B = {p2->img[r], p2->gx[r], p2->gy[r], p2->w[r], p2->h[r]};
      xl *= ss;
      yl *= ss;
      xo *= ss;
      yo *= ss;
      val = track_one_sums(xl, yl, &xo, &yo, &A, &B, P);
      if (val == SMALL_DET || val == OOB) break;
    }
    if (val == OOB || xo < P->borderx || xo > W - 1 - P->borderx || yo < P->bordery ||
        yo > H - 1 - P->bordery) {
      fx[k] = -1.0f;
      fy[k] = -1.0f;
      fval[k] = OOB;
    } else if (val != TRACKED) {
      fx[k] = -1.0f;
      fy[k] = -1.0f;
      fval[k] = val;
    } else {
      fx[k] = xo;
      fy[k] = yo;
      fval[k] = TRACKED;
    }
  }

  if (P->sequentialMode)
    t->last = p2;
  else
    pyr_free(p2);
  pyr_free(p1);
}
