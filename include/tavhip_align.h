/* libtavhip, forced alignment -- the second public header of libtavhip.so.
 *
 * The reference's run_scripts/get_times.py aligns a transcript to the frames of a wav2vec2 CTC model (get_trellis: T torch ops on the host
 * per utterance, backtrack: a Python loop over the trellis) to get the (start, end) seconds its clips are cut with.  The entry points below
 * are that step on the device.  They follow the rules of include/tavhip.h (extern "C", device pointers and sizes, `stream` a hipStream_t
 * passed as void*, no allocation, no synchronisation, TAV_ERR_* codes) and live in the same shared object.  They have a header of their own
 * because the symbol set of tavhip.h is pinned by a recorded table (tests/golden/entry_plan_golden.json); a change that re-records the
 * table may fold this header in.  tav_align_version() is bumped on any signature change here.
 */
#ifndef TAVHIP_ALIGN_H
#define TAVHIP_ALIGN_H
#include <stdint.h>
#include "tavhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int tav_align_version(void);

/* out[r][c] = log_softmax(logits[r][0..V))[c] for c < V; columns [V, ld_out) are not written and columns [V, ld_in) are not read (a
 * 29-label head computed 32 wide keeps its pad columns out of the sum).  f32, one wave per row; max, sum and log in f32 in an order that
 * does not depend on the launch.  ld_in, ld_out >= V. */
int tav_ctc_log_softmax(const float* logits, float* out, int64_t R, int64_t V, int64_t ld_in, int64_t ld_out, void* stream);

/* The launch plan for a batch whose longest row has T frames and N tokens over V labels (host arithmetic). */
typedef struct tav_align_plan {
    int32_t block;              /* threads of the workgroup (one workgroup per utterance)                                     */
    int32_t tokens_per_thread;  /* trellis columns a thread keeps in registers: block * tokens_per_thread >= N + 1             */
    int32_t frames_per_stage;   /* emission rows of one LDS stage (two stages: the next one is loaded under the current one)    */
    int32_t bits_frames;        /* frames whose decision words fit LDS; < T means the words go through the workspace            */
    int64_t lds_bytes;          /* dynamic LDS of the launch                                                                   */
    int64_t ws_bytes_per_row;   /* workspace bytes per utterance, 0 when the decision words stay in LDS                        */
} tav_align_plan;
int tav_ctc_align_plan(int64_t T, int64_t N, int64_t V, tav_align_plan* plan);
/* Workspace bytes of a batch of B (0 when none is needed, negative TAV_ERR_* for a refused shape). */
int64_t tav_ctc_align_ws_bytes(int64_t B, int64_t T, int64_t N, int64_t V);

/* CTC forced alignment of B utterances, one workgroup each (get_times.py: get_trellis + backtrack + the grouping of merge_repeats).
 *   tr[0][0] = 0, tr[0][j>0] = -inf, tr[t+1][0] = 0, tr[t+1][j] = max(tr[t][j] + e[t][blank], tr[t][j-1] + e[t][tok[j-1]])
 * then, in the same launch, the walk back from the smallest t that maximises tr[t][N_b], taking `changed > stayed` (a tie stays) until
 * j reaches 0.  Row b uses its first n_frames[b] frames and n_tokens[b] tokens (both clamped into [0, Tmax] / [0, Nmax]).
 * Every output row is written in full, except the optional trellis, which is written for t <= T_b, j <= N_b only.
 *   path_token[b][t]  token index on the path's frames, -1 elsewhere
 *   path_prob[b][t]   exp of the emission the step took (the token's if it changed, the blank's if it stayed), 0.0 off the path
 *   seg[b][j]         {first frame, one past the last frame} of token j; {-1, -1} for j >= N_b or a failed row
 *   seg_score[b][j]   f64 sum of the token's path_prob in ascending frame order / count, rounded once; 0.0 where seg is -1
 *   span[b]           {first frame, one past the last frame, points, status}; status bit 0: failed to align (the reference raises
 *                     ValueError; the first three are then -1, -1, 0), bit 1: a token id outside [0, V) was clamped
 * workspace: tav_ctc_align_ws_bytes(B, Tmax, Nmax, V) bytes, may be NULL when that is 0. */
typedef struct tav_ctc_align_args {
    const float* emission;      /* [B][Tmax][ld] f32 log-probabilities, V valid columns */
    const int32_t* tokens;      /* [B][Nmax] */
    const int32_t* n_frames;    /* [B] */
    const int32_t* n_tokens;    /* [B] */
    float* trellis;             /* optional [B][Tmax + 1][Nmax + 1] */
    int32_t* path_token;        /* [B][Tmax] */
    float* path_prob;           /* [B][Tmax] */
    int32_t* seg;               /* [B][Nmax][2] */
    float* seg_score;           /* [B][Nmax] */
    int32_t* span;              /* [B][4] */
    void* workspace;
    int64_t workspace_bytes;
    int64_t B, Tmax, Nmax, V, ld;
    int32_t blank_id;
    int32_t reserved;
} tav_ctc_align_args;
int tav_ctc_align(const tav_ctc_align_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
