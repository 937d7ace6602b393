/*
 * bsw_early_ref.c — the scalar banded-SW extension loop of oracle/bsw_oracle.c restated with the early-exit rule of
 * csrc/bsw_extend.hip ("BSW kernel: the early exit"), and the two task families of
 * tests/test_bsw_early_exit_cases.py.  TEST INFRASTRUCTURE ONLY: compiled by the tests with the host compiler.
 *
 * The rule, after row i is complete (gscore, max, the z-drop test and the next row's trimmed beg / end all done):
 *     P = max of  row[j].h + a * (qlen - j)        over the columns j of [rbeg, rend] with row[j].h > 0
 *                 row[j].e + a * (qlen - 1 - j)    over the columns j of [rbeg, rend] with row[j].e > 0
 *                 hb + a * qlen                    if beg == 0 and hb = h0 - o_del - e_del * (i + 2) > 0
 * with a the largest entry of the scoring matrix and [rbeg, rend] the band of row i; the task ends if P <= max and P < gscore.
 * It is applied only while every stored cell to the right of rend is zero (the zero-tail column zr).
 *
 * mode 0: the rule off (the oracle's loop); 1: tested after every row; 2: only after rows with (i & 3) == 3; 3: a WRONG rule,
 * P <= gscore in place of P < gscore, with which the tests pick the tasks where a later row ties gscore and gtle must move.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "bwams_types.h"

typedef struct { int32_t h, e; } cell_t;

static int early_scalar(const bwams_sw_opt_t *o, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int32_t w, int h0,
                        int mode, int *qle, int *tle, int *gtle, int *gscore_out, int *max_off_out, int64_t *cells, int32_t *rows,
                        uint8_t *by_rule)
{
    const int m = 5;
    const int o_del = o->o_del, e_del = o->e_del, o_ins = o->o_ins, e_ins = o->e_ins;
    const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
    int i, j, k;

    int8_t *qp = (int8_t *)malloc((size_t)(qlen > 0 ? qlen : 1) * m);
    cell_t *row = (cell_t *)calloc((size_t)qlen + 1, sizeof(cell_t));
    for (k = i = 0; k < m; ++k) {
        const int8_t *p = &o->mat[k * m];
        for (j = 0; j < qlen; ++j) qp[i++] = p[query[j]];
    }
    row[0].h = h0;
    if (qlen >= 1) row[1].h = h0 > oe_ins ? h0 - oe_ins : 0;
    for (j = 2; j <= qlen && row[j - 1].h > e_ins; ++j) row[j].h = row[j - 1].h - e_ins;
    int zr = -1;                              /* the zero tail: every stored cell of a column > zr is zero */
    for (j = 0; j <= qlen; ++j) if (row[j].h > 0) zr = j;

    int a = 0;
    for (i = 0; i < m * m; ++i) a = a > o->mat[i] ? a : o->mat[i];
    int max_ins = (int)((double)(qlen * a + o->end_bonus - o_ins) / e_ins + 1.);
    if (max_ins < 1) max_ins = 1;
    if (w > max_ins) w = max_ins;
    int max_del = (int)((double)(qlen * a + o->end_bonus - o_del) / e_del + 1.);
    if (max_del < 1) max_del = 1;
    if (w > max_del) w = max_del;

    int max = h0, max_i = -1, max_j = -1, max_ie = -1, gscore = -1, max_off = 0;
    int beg = 0, end = qlen;
    *by_rule = 0;
    for (i = 0; i < tlen; ++i) {
        int f = 0, h1, rmax = 0, mj = -1;
        const int8_t *q = &qp[target[i] * qlen];
        if (beg < i - w) beg = i - w;
        if (end > i + w + 1) end = i + w + 1;
        if (end > qlen) end = qlen;
        if (beg == 0) {
            h1 = h0 - (o_del + e_del * (i + 1));
            if (h1 < 0) h1 = 0;
        } else h1 = 0;
        for (j = beg; j < end; ++j) {
            cell_t *p = &row[j];
            int M = p->h, e = p->e, h, t;
            p->h = h1;
            M = M ? M + q[j] : 0;
            h = M > e ? M : e;
            h = h > f ? h : f;
            h1 = h;
            mj = rmax > h ? mj : j;
            rmax = rmax > h ? rmax : h;
            t = M - oe_del; t = t > 0 ? t : 0;
            e -= e_del;     e = e > t ? e : t;
            p->e = e;
            t = M - oe_ins; t = t > 0 ? t : 0;
            f -= e_ins;     f = f > t ? f : t;
            ++*cells;
        }
        row[end].h = h1; row[end].e = 0;
        ++*rows;
        if (j == qlen) {
            max_ie = gscore > h1 ? max_ie : i;
            gscore = gscore > h1 ? gscore : h1;
        }
        if (rmax == 0) break;
        if (rmax > max) {
            max = rmax; max_i = i; max_j = mj;
            int d = mj - i; if (d < 0) d = -d;
            max_off = max_off > d ? max_off : d;
        } else if (o->zdrop > 0) {
            if (i - max_i > mj - max_j) {
                if (max - rmax - ((i - max_i) - (mj - max_j)) * e_del > o->zdrop) break;
            } else {
                if (max - rmax - ((mj - max_j) - (i - max_i)) * e_ins > o->zdrop) break;
            }
        }
        const int rbeg = beg, rend = end;
        for (j = beg; j < end && row[j].h == 0 && row[j].e == 0; ++j) {}
        beg = j;
        for (j = end; j >= beg && row[j].h == 0 && row[j].e == 0; --j) {}
        end = j + 2 < qlen ? j + 2 : qlen;
        /* ---- the rule */
        const int tail_known = rend >= zr;            /* nothing alive to the right of this row's band */
        if (tail_known) zr = j;                       /* the last non-zero column the trim found (beg - 1: none) */
        if (mode && a > 0 && tail_known && (mode != 2 || (i & 3) == 3)) {
            int P = 0, t;
            for (j = rbeg; j <= rend; ++j) {
                if (row[j].h > 0) { t = row[j].h + a * (qlen - j); P = P > t ? P : t; }
                if (row[j].e > 0) { t = row[j].e + a * (qlen - 1 - j); P = P > t ? P : t; }
            }
            if (beg == 0) {
                const int hb = h0 - o_del - e_del * (i + 2);
                if (hb > 0) { t = hb + a * qlen; P = P > t ? P : t; }
            }
            if (P <= max && (mode == 3 ? P <= gscore : P < gscore)) { *by_rule = 1; break; }
        }
    }
    free(row); free(qp);
    *qle = max_j + 1; *tle = max_i + 1; *gtle = max_ie + 1; *gscore_out = gscore; *max_off_out = max_off;
    return max;
}

/* the six outputs into pairs[]; per task the cells computed, the rows walked and whether the rule ended it */
void bsw_early_pairs(const bwams_sw_opt_t *o, bwams_seqpair_t *pairs, const uint8_t *ref, const uint8_t *qer, int64_t n, int32_t w,
                     int32_t mode, int64_t *cells, int32_t *rows, uint8_t *by_rule)
{
    for (int64_t i = 0; i < n; ++i) {
        bwams_seqpair_t *p = &pairs[i];
        cells[i] = 0; rows[i] = 0;
        p->score = early_scalar(o, p->len2, qer + p->idq, p->len1, ref + p->idr, w, p->h0, mode, &p->qle, &p->tle, &p->gtle,
                                &p->gscore, &p->max_off, &cells[i], &rows[i], &by_rule[i]);
    }
}

/* ---- the task families -------------------------------------------------------------------------------------------------- */
static uint64_t rng_next(uint64_t *s) { uint64_t x = *s; x ^= x << 13; x ^= x >> 7; x ^= x << 17; *s = x; return x * 0x2545F4914F6CDD1Dull; }
static uint32_t rng_below(uint64_t *s, uint32_t n) { return (uint32_t)((rng_next(s) >> 33) % n); }
static double rng_unit(uint64_t *s) { return (double)(rng_next(s) >> 11) / 9007199254740992.0; }

static void put_task(bwams_seqpair_t *p, int64_t k, int64_t ro, int64_t qo, int tl, int ql, int h0)
{
    memset(p, 0, sizeof *p);
    p->idr = (int32_t)ro; p->idq = (int32_t)qo; p->id = (int32_t)k; p->len1 = tl; p->len2 = ql; p->h0 = h0;
    p->seqid = (int32_t)(k / 3); p->regid = (int32_t)(k % 3);
}

/* Reads of 150 bases drawn from random text with the simulator's error profile (substitution rate one of 0, 0, 0.5, 2, 5 %, indels a
 * fifth of it); the longest exact run is the seed, and its left and right extensions are the tasks: the target is
 * qlen + max_gap(qlen) bases of the text (max_gap as cal_max_gap with a = 1, gap costs 6 / 1, w = 100), h0 the seed's length
 * (the right task: plus the bases to the left, as after an exact left extension).  One read in six is a chance hit: the text on
 * both sides of its seed is unrelated to the read, so its tasks die within a few rows on their own.  Returns the number of tasks written (<= cap),
 * ref / qer need cap * 400 / cap * 150 bytes. */
int64_t bsw_early_gen_reads(uint64_t seed, int64_t cap, bwams_seqpair_t *pairs, uint8_t *ref, uint8_t *qer)
{
    enum { TEXT = 1 << 16, RL = 150 };
    static const double kSub[5] = {0., 0., 0.005, 0.02, 0.05};
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    uint8_t *text = (uint8_t *)malloc(TEXT);
    for (int i = 0; i < TEXT; ++i) text[i] = (uint8_t)rng_below(&s, 4);
    int64_t n = 0, ro = 0, qo = 0;
    while (n + 2 <= cap) {
        const double sub = kSub[rng_below(&s, 5)], indel = sub / 5.;
        const int start = 1000 + (int)rng_below(&s, TEXT - 2000);
        uint8_t read[RL];
        int rpos[RL];                                   /* text position a read base was copied from, -1: not a copy */
        int t = start, l = 0;
        while (l < RL) {
            const double u = rng_unit(&s);
            if (u < sub) { read[l] = (uint8_t)((text[t] + 1 + rng_below(&s, 3)) & 3); rpos[l++] = -1; ++t; }
            else if (u < sub + indel / 2) ++t;                                                   /* deletion from the read */
            else if (u < sub + indel) { read[l] = (uint8_t)rng_below(&s, 4); rpos[l++] = -1; }   /* insertion */
            else { read[l] = text[t]; rpos[l++] = t++; }
        }
        int best = 0, bq = 0, run = 0;
        for (int i = 0; i < RL; ++i) {
            run = (rpos[i] >= 0 && i && rpos[i - 1] >= 0 && rpos[i] == rpos[i - 1] + 1) ? run + 1 : (rpos[i] >= 0 ? 1 : 0);
            if (run > best) { best = run; bq = i - run + 1; }
        }
        if (best < 19) continue;
        const int qb = bq, qe = bq + best;
        int rb = rpos[bq], re = rb + best;
        if (rng_below(&s, 6) == 0) { rb = 1000 + (int)rng_below(&s, TEXT - 2000); re = 1000 + (int)rng_below(&s, TEXT - 2000); }
        for (int side = 0; side < 2; ++side) {
            const int ql = side ? RL - qe : qb;
            if (ql == 0) continue;
            int gap = ql - 6 + 1;
            gap = gap < 1 ? 1 : (gap > 200 ? 200 : gap);
            const int tl = ql + gap;
            for (int i = 0; i < ql; ++i) qer[qo + i] = side ? read[qe + i] : read[qb - 1 - i];
            for (int i = 0; i < tl; ++i) ref[ro + i] = side ? text[re + i] : text[rb - 1 - i];
            put_task(&pairs[n], n, ro, qo, tl, ql, side ? best + qb : best);
            ro += tl; qo += ql; ++n;
        }
    }
    free(text);
    return n;
}

/* Adversarial tasks: alphabets of 1 to 4 letters, qlen 1 .. 160, tlen 1 .. 330, h0 1 .. 200; the query is random, or a copy of the
 * target read along a shifted and drifting diagonal (every `drift` bases the copy skips or repeats a base), with substitutions and Ns
 * in both.  ref / qer need n * 330 / n * 160 bytes. */
void bsw_early_gen_adversarial(uint64_t seed, int64_t n, bwams_seqpair_t *pairs, uint8_t *ref, uint8_t *qer)
{
    uint64_t s = seed * 0xD1B54A32D192ED03ull + 7;
    int64_t ro = 0, qo = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int sigma = 1 + (int)rng_below(&s, 4);
        const int ql = 1 + (int)rng_below(&s, 160), tl = 1 + (int)rng_below(&s, 330);
        const int h0 = rng_below(&s, 4) ? 1 + (int)rng_below(&s, 200) : 1 + (int)rng_below(&s, 12);
        uint8_t *t = ref + ro, *q = qer + qo;
        for (int i = 0; i < tl; ++i) t[i] = (uint8_t)rng_below(&s, (uint32_t)sigma);
        const int kind = (int)rng_below(&s, 4);
        if (kind == 0) {
            for (int i = 0; i < ql; ++i) q[i] = (uint8_t)rng_below(&s, (uint32_t)sigma);
        } else {
            int p = kind == 1 ? 0 : (int)rng_below(&s, 24) - 8;                  /* the shift of the diagonal */
            const int drift = kind == 3 ? 3 + (int)rng_below(&s, 40) : 1 << 30;
            const int dir = rng_below(&s, 2) ? 1 : -1;
            const double sub = (double)rng_below(&s, 4) * 0.03;
            for (int i = 0; i < ql; ++i) {
                if (i && i % drift == 0) p += dir;
                const int tp = i + p;
                q[i] = tp >= 0 && tp < tl ? t[tp] : (uint8_t)rng_below(&s, (uint32_t)sigma);
                if (rng_unit(&s) < sub) q[i] = (uint8_t)rng_below(&s, 4);
            }
        }
        if (rng_below(&s, 8) == 0) q[rng_below(&s, (uint32_t)ql)] = 4;
        if (rng_below(&s, 8) == 0) { const int at = (int)rng_below(&s, (uint32_t)tl), len = 1 + (int)rng_below(&s, 5); for (int i = at; i < tl && i < at + len; ++i) t[i] = 4; }
        put_task(&pairs[k], k, ro, qo, tl, ql, h0);
        ro += tl; qo += ql;
    }
}
