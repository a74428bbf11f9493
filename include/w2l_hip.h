/*
 * w2l_hip.h -- C ABI of libw2l_hip.so: the MI355X (gfx950) implementation of the
 * wav2letter acoustic-training hot path.
 *
 * Every pointer is a DEVICE pointer unless its name starts with h_.  All entry
 * points are asynchronous on `stream` (a hipStream_t passed as void*; NULL =
 * the default stream), re-entrant, keep no global state and return a
 * w2l_status (0 = OK) instead of throwing.  The caller owns every buffer,
 * including the workspaces sized by the *_workspace_size queries.
 *
 * Section 1 mirrors, one for one, the static functions of Flashlight's
 *   fl::lib::{cpu,cuda}::{ForceAlignmentCriterion, FullConnectionCriterion,
 *   ViterbiPath, ConnectionistTemporalClassificationCriterion}<float>
 *   and CriterionUtils (flashlight/lib/sequence/criterion/, un-vendored; call
 *   sites in /root/reference: recipes/slimIPL/src/Train.cpp:406-410, :1675,
 *   :838, :1375; recipes/joint_training_vox_populi/cpc/Train.cpp:813),
 * which is what fl::pkg::speech::{ASGLoss,CTCLoss} bind.
 * Layouts: emissions [B][T][N] (ArrayFire dims (N,T,B)); targets [B][L] int32
 * padded with negative values; transitions [N][N] indexed [to][from]; CTC
 * blank = N-1; paths [B][T] int32.
 */
#ifndef W2L_HIP_H_
#define W2L_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* w2l_stream_t; /* hipStream_t */

typedef enum {
  W2L_OK = 0,
  W2L_EINVAL = 1,       /* bad shape / null pointer (Flashlight throws std::invalid_argument) */
  W2L_EHIP = 2,         /* a HIP runtime call failed; see w2l_last_hip_error() */
  W2L_EUNSUPPORTED = 3  /* shape outside what this build implements */
} w2l_status;

/* fl::lib::seq::CriterionScaleMode (selected by --onorm / --sqnorm,
 * recipes/slimIPL/src/Train.cpp:389; recipes/conv_glu/librispeech/train.cfg:20-21) */
typedef enum {
  W2L_SCALE_NONE = 0,
  W2L_SCALE_INPUT_SZ = 1,
  W2L_SCALE_INPUT_SZ_SQRT = 2,
  W2L_SCALE_TARGET_SZ = 3,
  W2L_SCALE_TARGET_SZ_SQRT = 4
} w2l_scale_mode;

const char* w2l_version(void);
int w2l_last_hip_error(void); /* hipError_t of the last failing call on this thread */

/* ------------------------------------------------------------------------
 * 1. Sequence criteria
 * ---------------------------------------------------------------------- */

/* CriterionUtils::batchTargetSize: targetSize[b] = #leading non-negative labels
 * of target[b][0..L), clamped to maxSize (== T for ASG). */
int w2l_batch_target_size(int B, int L, int maxSize, const int* target, int* targetSize,
                          w2l_stream_t stream);
/* CTC flavour: with R = adjacent repeats, L <- min(L + R, T) - R */
int w2l_batch_ctc_target_size(int B, int L, int T, const int* target, int* targetSize,
                              w2l_stream_t stream);

/* FullConnectionCriterion<float>: log-partition over all N^T paths. */
size_t w2l_fcc_workspace_size(int B, int T, int N);
int w2l_fcc_forward(int B, int T, int N, int scaleMode, const float* input,
                    const int* targetSize, const float* trans, float* loss,
                    void* workspace, w2l_stream_t stream);
/* inputGrad [B][T][N] and transGrad [N][N] are OVERWRITTEN (transGrad summed over b). */
int w2l_fcc_backward(int B, int T, int N, const float* trans, const float* grad,
                     float* inputGrad, float* transGrad, void* workspace,
                     w2l_stream_t stream);

/* ForceAlignmentCriterion<float>: log-sum over monotone alignments of target. */
size_t w2l_fac_workspace_size(int B, int T, int N, int L);
int w2l_fac_forward(int B, int T, int N, int L, int scaleMode, const float* input,
                    const int* target, const int* targetSize, const float* trans,
                    float* loss, void* workspace, w2l_stream_t stream);
int w2l_fac_backward(int B, int T, int N, int L, const int* target, const int* targetSize,
                     const float* grad, float* inputGrad, float* transGrad,
                     void* workspace, w2l_stream_t stream);
/* forced alignment; bestPaths [B][T] holds target labels */
int w2l_fac_viterbi(int B, int T, int N, int L, const float* input, const int* target,
                    const int* targetSize, const float* trans, int* bestPaths,
                    void* workspace, w2l_stream_t stream);
/* AutoSegmentationCriterion in ONE call: loss[b] = FullConnectionCriterion - ForceAlignmentCriterion, the composition
 * fl::pkg::speech::ASGLoss::forward makes of the two criteria above (constructed at recipes/slimIPL/src/Train.cpp:408-410, run at
 * :1675, backward at :1720; math SURVEY App. B.1 / B.2).  target is the [B][L] batch as the Trainer hands it over (padded with
 * negative labels; the target sizes are counted on the device), trans the shared [N][N] transition parameter.  The two criteria
 * run side by side on `stream` and a library-owned side stream of the device; for the letter-sized label sets (N <= 31, L <= 320)
 * the launches that exist only to glue two calls together (target sizes, the loss / gradient differences) ride on their
 * neighbours (csrc/criterion_asg_fused.hpp).  backward OVERWRITES inputGrad [B][T][N] and transGrad [N][N] with the gradients of
 * sum_b grad[b] loss[b]; it needs the workspace of the forward call of the same batch.  Results equal the composed calls bit for bit. */
size_t w2l_asg_workspace_size(int B, int T, int N, int L);
int w2l_asg_forward(int B, int T, int N, int L, int scaleMode, const float* input, const int* target, const float* trans,
                    float* loss, void* workspace, w2l_stream_t stream);
int w2l_asg_backward(int B, int T, int N, int L, const int* target, const float* trans, const float* grad, float* inputGrad,
                     float* transGrad, void* workspace, w2l_stream_t stream);
/* Range check (diagnostics; no counterpart in the reference, whose log-domain recursion -- SURVEY App. B.1 / B.2, call sites
 * recipes/slimIPL/src/Train.cpp:408-410, :1675 -- is what the flagged utterances are recomputed with).  The fp32 / fp64
 * scaled-domain scans behind w2l_fcc_forward / w2l_fac_forward check per utterance that their inputs stay inside what they hold
 * exactly and hand the rest to log-domain kernels inside the same call: results are exact either way.  flags[b] (device, [B]) = 1
 * when utterance b of the LAST forward call on `workspace` (same B, T, N[, L]) took the log-domain path, else 0. */
int w2l_fcc_range_flags(int B, int T, int N, const void* workspace, int* flags, w2l_stream_t stream);
int w2l_fac_range_flags(int B, int T, int N, int L, const void* workspace, int* flags, w2l_stream_t stream);

/* LinSegCriterion (recipes/slimIPL/src/Train.cpp:589-617, --linseg): ASG on the target stretched linearly over the
 * T frames.  Flashlight getLinearTarget [UNVENDORED]: linTarget[b][t] = target[b][t * L_b / T], L_b = leading
 * non-negative entries of target[b][0..L); a row with L_b == 0 or L_b > T is filled with -1. */
int w2l_linear_target(int B, int L, int T, const int* target, int* linTarget /*[B][T]*/,
                      w2l_stream_t stream);
/* ForceAlignmentCriterion<float> on a length-T target (one alignment: label path[b][t] at frame t):
 * loss[b] = s_b * (sum_t input[b][t][y_t] + sum_{t>=1} trans[y_t][y_{t-1}]), target size = T in s_b.
 * A row of -1 gives loss 0 and zero gradients (as w2l_fac_* do for an empty target). */
int w2l_fac_fullpath_forward(int B, int T, int N, int scaleMode, const float* input,
                             const int* path, const float* trans, float* loss,
                             w2l_stream_t stream);
/* inputGrad [B][T][N] and transGrad [N][N] are OVERWRITTEN (transGrad summed over b; bit-reproducible
 * for N <= 64, float atomics above). */
int w2l_fac_fullpath_backward(int B, int T, int N, int scaleMode, const int* path,
                              const float* grad, float* inputGrad, float* transGrad,
                              w2l_stream_t stream);

/* ViterbiPath<float>: max-product path, first-max tie break, BIT-EXACT with the
 * CPU recursion (fp32 adds in the order (delta[j] + trans[i][j]) + x[t][i]). */
size_t w2l_viterbi_workspace_size(int B, int T, int N);
int w2l_viterbi_compute(int B, int T, int N, const float* input, const float* trans,
                        int* path, void* workspace, w2l_stream_t stream);

/* ConnectionistTemporalClassificationCriterion<float>; input are raw emissions
 * (log-softmax is applied inside), blank = N-1. */
size_t w2l_ctc_workspace_size(int B, int T, int N, int L);
int w2l_ctc_forward(int B, int T, int N, int L, int scaleMode, const float* input,
                    const int* target, const int* targetSize, float* loss,
                    void* workspace, w2l_stream_t stream);
/* needs `input` again (the softmax is recomputed instead of stored: 12*B*T*N
 * bytes of HBM traffic per fwd+bwd instead of 16). inputGrad OVERWRITTEN. */
int w2l_ctc_backward(int B, int T, int N, int L, const float* input, const int* target,
                     const int* targetSize, const float* grad, float* inputGrad,
                     void* workspace, w2l_stream_t stream);
/* CTCLoss::viterbiPath: per-frame argmax, first max wins */
int w2l_ctc_viterbi(int B, int T, int N, const float* input, int* path, w2l_stream_t stream);
/* Evaluation in one read of the emissions: loss [B] bitwise equal to w2l_ctc_forward's (+inf for an infeasible target) and
 * path [B][T] bitwise equal to w2l_ctc_viterbi's.  Keeps nothing for a backward pass: the workspace holds the per-frame lse and
 * label probabilities only (no alpha / beta rows, exponents or label links), so w2l_ctc_backward cannot follow this call.
 * w2l_ctc_score_workspace_size is host arithmetic and smaller than w2l_ctc_workspace_size for the same shape.
 * L > 1023: W2L_EUNSUPPORTED, as w2l_ctc_forward. */
size_t w2l_ctc_score_workspace_size(int B, int T, int N, int L);
int w2l_ctc_score(int B, int T, int N, int L, int scaleMode, const float* input, const int* target,
                  const int* targetSize, float* loss, int* path, void* workspace, w2l_stream_t stream);
/* Forced alignment: the most probable lattice path of a KNOWN transcript, one label per frame (blank = N-1).
 *   frames [B]: emission frames that belong to utterance b, 1..T (NULL: T for all); path[b][t] = N-1 for frames[b] <= t < T.
 *   targetSize as w2l_batch_ctc_target_size(B, L, T, ...) writes it.  A row whose L_b labels with R adjacent equal pairs do not fit
 *   (L_b + R > frames[b]) gets path -1 everywhere and score -inf; L_b = 0 gives all blank.
 *   path is BIT-EXACT with the max-plus recursion on the RAW emissions, a'[s] = max(stay, advance, skip) + x[t][ext[s]] with one
 *   fp32 add, candidates in the order stay, advance, skip, a later one winning only when strictly greater (w2l_fac_viterbi's rule);
 *   end state 2 L_b, replaced by 2 L_b - 1 only when strictly greater.  (A per-frame constant cannot change the arg-max, so the
 *   path is also the best one under the log-softmax.)
 *   score [B] (may be NULL): sum over t < frames[b] of log_softmax(x[t])[path[t]], accumulated in double.  With score == NULL the
 *   call reads only the L_b + 1 label emissions of every frame.
 * w2l_ctc_align_workspace_size is host arithmetic.  L > 1023: W2L_EUNSUPPORTED, as w2l_ctc_forward. */
size_t w2l_ctc_align_workspace_size(int B, int T, int N, int L);
int w2l_ctc_align(int B, int T, int N, int L, const float* input, const int* target, const int* targetSize,
                  const int* frames, int* path, float* score, void* workspace, w2l_stream_t stream);
/* CTC prefix beam search without lexicon or LM, n-best output.  Blank is N-1; `frames` as in w2l_ctc_align.
 * For utterance b, with F = frames[b]:
 *   Frame scores.  normalize = 0: lp_t[c] = x[t][c] (the raw emission); normalize = 1: lp_t[c] = x[t][c] - lse_t in fp32.
 *   Frame tokens.  The K non-blank classes with the largest lp_t, ordered by lp descending, then class index ascending.
 *     K larger than N-1 is clipped to N-1.
 *   State.  A beam of at most W entries ordered by rank 0, 1, ...  An entry is a label prefix with last label e and two values:
 *     pb (alignments ending in blank) and pnb (alignments ending in e); tot = pb (+) pnb, where (+) is log(exp a + exp b) when
 *     logAdd = 1 and max when logAdd = 0.  The beam starts as the empty prefix with pb = 0, pnb = -inf.
 *   Candidates of frame t.  For the entry of rank r:
 *     stay(r): pb' = lp[blank] + tot; pnb' = lp[e] + pnb for a non-empty prefix (lp[e] is read from the row even when e is not
 *       among the frame's tokens), -inf for the empty prefix.
 *     ext(r, k), k-th frame token c: pb' = -inf, pnb' = lp[c] + (c == e ? pb : tot).
 *   Merge.  If ext(r, k) spells the prefix of a beam entry j (j's parent is entry r's prefix and j's last label is c), its pnb'
 *     is (+)-ed into stay(j).pnb' and the extension itself disappears: no two entries ever spell the same prefix.
 *   Prune.  Candidates whose total is -inf are dropped, then those with total < best - threshold (threshold >= 0; +inf: no
 *     pruning).  The first W candidates in this order are kept: total descending, then r ascending, then stay before extension,
 *     then k ascending (a merged candidate carries the key of its stay).  That order defines the ranks of the next beam.
 *   Output.  After frame F-1 the first M entries in rank order: lengths[b][m] the true label count, labels[b][m] the first
 *     min(length, Lmax) labels and -1 beyond, scores[b][m] = tot.  Rows beyond the surviving entries: length -1, score -inf,
 *     labels -1.
 * With logAdd = 0 every value is one fp32 add of two stored values, or a compare: the result is reproducible bit for bit, ties
 * included; the one exception is the sign of a zero: a new extension's pnb is stored as recovered from its selection key, which
 * carries -0 as +0 (the two compare equal, so no decision and no non-zero value depends on it).  With logAdd = 1 the (+) is fp32
 * (expf / log1pf).
 * Limits: W in 1..64, K after clipping <= 64 (beyond: W2L_EUNSUPPORTED); 1 <= M <= W, N >= 2, Lmax >= 1, threshold not NaN and
 * >= 0, non-null pointers other than frames (else W2L_EINVAL).  All argument checks return before anything touches the device.
 * frames is device memory and therefore NOT checked: a value outside 1..T is clamped into 1..T, as in w2l_ctc_align.
 * w2l_ctc_beam_workspace_size is host arithmetic (0 for arguments the search refuses). */
size_t w2l_ctc_beam_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                        int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                        int nbest /*M*/, int maxLen /*Lmax*/,
                        int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                        void* workspace, w2l_stream_t stream);
/* Back-off n-gram language model over the token dictionary, as a table.  Host only: none of w2l_ngram_lm_* touches the GPU.
 * Refusals set a message for w2l_host_last_error().
 *   Words.  0 .. numTokens-1 are the token classes (numTokens = N-1 for a search over N classes), numTokens is BOS, numTokens+1
 *     is EOS.  <unk> is only a fallback log-probability, unkLogp.  Values are fp32 natural logs.
 *   States.  State 0 is the empty context; every n-gram of order below the model order is a state with a back-off weight bo[s]
 *     and a suffix state suf[s], the state of the longest proper suffix of its words that is a state (its context with the first
 *     word dropped, in a model that lists every suffix).  The start state is the state of (BOS); 0 when the model has no BOS
 *     unigram or is of order 1.
 *   Edges.  (state, word) -> (log p, next): one per n-gram, from the state of its context.  next is the n-gram's own state, or,
 *     for an n-gram of the model order, the state of its longest proper suffix that is a state.
 *   Score rule, every add one fp32 add in this order:
 *       q(s, w):  acc = 0
 *                 loop: if edge (s, w) exists: return (acc + p, next)
 *                       if s == 0:             return (acc + unkLogp, 0)
 *                       acc = acc + bo[s];  s = suf[s]
 *   Blob.  One position-independent block (offsets, no pointers; layout in csrc/ngram_lm.hpp): the same bytes are the table on the
 *     host and, after one copy, on the device.  Edge lookup is an open-addressing hash at load factor <= 1/2.  The memory holding
 *     a blob must be 16-byte aligned.
 * w2l_ngram_lm_build: n-grams per order, concatenated: counts[order]; words: counts[0] 1-grams, then counts[1] 2-grams (2 ints
 *   each), ...; logp and backoff one value per n-gram in the same sequence (backoff may be NULL: all 0; the top order's are
 *   ignored).  Two calls: blob = NULL writes the size to *blobBytes; then *blobBytes is the room of blob and becomes the size.
 *   W2L_EINVAL: an n-gram whose context is not itself an n-gram, a duplicate n-gram, a word id outside 0 .. numTokens+1, a
 *   non-finite value, too little room.  W2L_EUNSUPPORTED: order above 8.
 * w2l_ngram_lm_from_arpa: ARPA text -> blob (the same two calls); tokens[i] is the spelling of class i.  log10 values become
 *   natural logs in double, rounded once to fp32.  <s>, </s> and <unk> are recognised (a token spelled like one of them wins);
 *   the <unk> unigram sets unkLogp; an n-gram with any other word that is no token is skipped, *skipped (may be NULL) and the
 *   message count them.  A class without unigram scores as <unk>; without <unk> too the load is refused and the message names the
 *   first such token.  Refused as well: a \data\ count that disagrees with its section, a file that ends before \end\, a
 *   KenLM binary (the message asks for the ARPA text), gzip.
 * w2l_ngram_lm_start / w2l_ngram_lm_score: the start state and q on a host blob (state and word are checked).
 * w2l_ngram_lm_info: any output may be NULL. */
int w2l_ngram_lm_build(int order, const size_t* counts, const int* words, const float* logp, const float* backoff,
                       int numTokens, float unkLogp, void* blob, size_t* blobBytes);
int w2l_ngram_lm_from_arpa(const char* path, int numTokens, const char* const* tokens, void* blob, size_t* blobBytes,
                           int* skipped);
int w2l_ngram_lm_info(const void* blob, int* order, int* numTokens, int* numStates, int* hasBos, int* hasEos);
int w2l_ngram_lm_start(const void* blob, int* state);
int w2l_ngram_lm_score(const void* blob, int state, int word, float* logp, int* next);
/* w2l_ctc_beam_search fused with an n-gram LM (lexicon-free: the LM's words are the token classes).  The contract is
 * w2l_ctc_beam_search's -- frame tokens by the acoustic lp alone, stay / ext / merge / prune / order / output -- with these changes:
 *   LM state.  Every entry carries the LM state of its prefix; the empty prefix has the start state.
 *   Extension.  ext(r, k) with token c:  pnb' = (lp[c] + (c == e ? pb : tot)) + g,  g = (lmWeight * q(s_r, c)) + classScore[c]:
 *     one fp32 multiply, one fp32 add (skipped when classScore is NULL), then the add to the acoustic sum.  The new entry's state
 *     is q's next state.
 *   Merge.  An extension merged into stay(j) contributes this pnb', g included: the entry it joins carries the same LM score, so
 *     every alignment of a prefix carries the prefix's LM score once.
 *   Prune and select act on totals that include g; the order is unchanged.
 *   End.  lmHasEos != 0 (what w2l_ngram_lm_info says of the blob): every surviving entry's score becomes
 *     tot + ((lmWeight * q(s, EOS)) + eosScore) and the entries are re-ranked by that score descending, then previous rank
 *     ascending.  lmHasEos == 0: no end term, and eosScore must be 0.
 *   lmScores[b][m]: the hypothesis's unweighted LM score: q added in label order from the start state in fp32 (0 + q1, + q2, ...),
 *     then + q(s, EOS) when lmHasEos; -inf for empty rows.
 * With logAdd = 0 the result is reproducible bit for bit as w2l_ctc_beam_search's is (same exception for the sign of a zero).
 * Limits and refusals: w2l_ctc_beam_search's, and lm or lmScores NULL, lmWeight or eosScore not finite, eosScore != 0 without
 * EOS (W2L_EINVAL), all before anything touches the device.  lm (a blob for N-1 tokens) and classScore [N-1] are device memory
 * and NOT checked: the kernel bounds every probe loop by the table's capacity, every back-off walk by its order and every state
 * by its state count, so a damaged table gives wrong scores, never a spin. */
size_t w2l_ctc_beam_lm_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_lm(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                           int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                           int nbest /*M*/, int maxLen /*Lmax*/, const void* lm, int lmHasEos, float lmWeight,
                           const float* classScore /*[N-1] or NULL*/, float eosScore,
                           int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                           float* lmScores /*[B][M]*/, void* workspace, w2l_stream_t stream);
/* The lexicon as a trie, one table.  Host only: none of w2l_lexicon_* touches the GPU.  Refusals set a message for
 * w2l_host_last_error().
 *   Nodes 0 .. numNodes-1, the root is 0, numbered in the order the spelling rows first reach them.  An edge (node, token) -> child
 *     is found through an open-addressing hash at load factor <= 1/2; every probe loop is bounded by the capacity.  A node stores
 *     smear (fp32), hasChildren, nw in 0..6 and up to 6 word ids: the first 6 words whose spelling ends at it, in row order.
 *   Blob.  One position-independent block (offsets, no pointers; layout in csrc/lexicon.hpp): the same bytes are the table on the
 *     host and, after one copy, on the device.  The memory holding a blob must be 16-byte aligned.
 * w2l_lexicon_build: numSpellings rows; row i spells word spellWord[i] with the tokens spellTokens[spellOff[i] .. spellOff[i+1]).
 *   Homophones (several words on one spelling) and several spellings of one word are rows like any other.  Words beyond the 6th of
 *   a node are dropped and counted in *dropped (may be NULL).  smear[v] is the exact max of wordSmear[w] over the words kept at v or
 *   below; wordSmear == NULL: all 0, no smearing.  silToken (-1: none) is the token the search lets loop at the root.  The two calls
 *   of w2l_ngram_lm_build: blob = NULL writes the size to *blobBytes; then *blobBytes is the room of blob and becomes the size.
 *   W2L_EINVAL: an empty spelling, a token outside 0 .. numTokens-1 (so blank cannot be spelled), a word id outside
 *   0 .. numWords-1, a duplicate (word, spelling) row, a spelling that begins with silToken, a non-finite smear value, too little
 *   room.  W2L_EUNSUPPORTED: 2^28 nodes or more.
 * w2l_lexicon_info (any output may be NULL), w2l_lexicon_child (*child = -1 when the edge is absent) and w2l_lexicon_node
 *   (words[6], -1 beyond nw; any output may be NULL) walk a host blob; node and token are checked. */
int w2l_lexicon_build(int numTokens, int numWords, size_t numSpellings, const int* spellWord, const size_t* spellOff,
                      const int* spellTokens, const float* wordSmear /*[numWords] or NULL*/, int silToken, void* blob,
                      size_t* blobBytes, size_t* dropped);
int w2l_lexicon_info(const void* blob, int* numTokens, int* numWords, int* numNodes, int* silToken, int* smeared);
int w2l_lexicon_child(const void* blob, int node, int token, int* child);
int w2l_lexicon_node(const void* blob, int node, float* smear, int* nw, int* words /*[6]*/, int* hasChildren);
/* w2l_ctc_beam_search restricted to the spellings of a lexicon, scored by an n-gram LM over WORDS (lm: a w2l_ngram_lm_* blob whose
 * "tokens" are the lexicon's numWords words) whose score is smeared down the trie (max smearing).  Like its siblings it is a PREFIX
 * search with pb / pnb: one hypothesis has one entry.  The contract is w2l_ctc_beam_search's -- frame tokens by the acoustic lp alone,
 * stay, (+), threshold, W, M, the output rows -- with these changes:
 *   State.  An entry is a hypothesis: a sequence of extensions.  Besides e, pb, pnb it carries its lexicon node u (the root at the
 *     start, after a completed word and after silence at the root), its LM state s, its word list and the unweighted LM sum acc;
 *     all four are functions of the hypothesis.
 *   Extensions of entry r by frame token k of class c, base = (c == e ? pb : tot):
 *     sil, slot 0: c == silToken and u is the root: pnb' = lp[c] + base; the new entry is at the root with state s; no word, no LM
 *       term.
 *     Otherwise v = child(u, c); without such a child (r, k) has no candidates.  a = (lp[c] + base) + (lmWeight * (smear[v] - su)),
 *       su = 0 at the root and smear[u] elsewhere: one fp32 subtract, one multiply, one add, in this order.
 *       in, slot 0: v has children: pnb' = a; the new entry is at v with state s.
 *       word i, slot 1+i, i < nw(v), w = words(v)[i]: pnb' = a + ((lmWeight * (q(s, w) - smear[v])) + wordScore); the new entry is
 *         at the root, its state is q's successor, w is appended, acc' = acc + q.
 *     Every extension has pb' = -inf.  In exact arithmetic the smear terms cancel when a word completes; in fp32 they leave their
 *     roundings: the contract is the operation sequence above.
 *   Merge.  A candidate is (+)-ed into stay(j).pnb' and disappears when j's parent hypothesis is entry r's hypothesis and j's last
 *     extension is the same one: the same token, the same resulting lexicon node and the same word or none.  Two hypotheses that
 *     spell the same tokens with different words, or with a different word boundary, are different entries.
 *   Order.  Total descending, r ascending, stay before extension, k ascending, slot ascending.
 *   End.  Entries whose node is not the root are dropped: only finished words count.  Then w2l_ctc_beam_search_lm's EOS term when
 *     lmHasEos (EOS is word numWords + 1 of the LM), the re-ranking by score descending, then previous rank ascending.  labels and
 *     lengths as before, silence tokens included; words[b][m] the first min(count, maxWords) word ids and -1 beyond;
 *     wordCounts[b][m] the true count, -1 for empty rows; lmScores as in the LM search.  When no entry is at the root, all M rows
 *     of the utterance are empty.
 * Not part of the contract: an unknown-word arc, log-add smearing.  (A silence score: the *_sil entry points below.)
 * With logAdd = 0 the result is reproducible bit for bit (same exception for the sign of a zero).
 * Limits and refusals: w2l_ctc_beam_search_lm's, and lexicon, words or wordCounts NULL, maxWords < 1, wordScore not finite
 * (W2L_EINVAL), all before anything touches the device.  lexicon and lm are device memory and NOT checked: the kernel bounds every
 * probe loop by the capacity, every back-off walk by the order and every node and state by its count, so a damaged table gives wrong
 * scores, never a spin. */
size_t w2l_ctc_beam_lex_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_lex(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                            int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                            int nbest /*M*/, int maxLen /*Lmax*/, const void* lm, int lmHasEos, float lmWeight,
                            const void* lexicon, float wordScore, float eosScore,
                            int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                            float* lmScores /*[B][M]*/, int maxWords, int* words /*[B][M][maxWords]*/, int* wordCounts /*[B][M]*/,
                            void* workspace, w2l_stream_t stream);
/* Beam search of an ASG model: w2l_asg_beam_search is lexicon-free with an optional token LM (the arguments of
 * w2l_ctc_beam_search_lm), w2l_asg_beam_search_lex uses a lexicon trie, a word LM and max smearing (the arguments of
 * w2l_ctc_beam_search_lex); both take trans, the criterion's transition matrix A [N][N], to x from, on the device.  The contract is
 * the CTC family's -- frame tokens, (+), threshold, W, M, order, tie key, output rows, frames, one prefix or hypothesis one entry --
 * with these changes:
 *   Classes.  There is no blank: all N classes are tokens.  K is clipped to N; an LM blob is over N tokens (EOS is word N + 1), a
 *     lexicon over N tokens; classScore is [N].
 *   State.  An entry has one value p and its last label e.  The beam starts as the empty prefix with p = 0.
 *   stay(r): p' = (p + A[e][e]) + lp[e]: two fp32 adds in this order, w2l_viterbi_compute's, so scores compare bit for bit; lp[e] is
 *     read from the row whether or not e is a frame token.  The empty prefix has no stay (-inf).
 *   ext(r, k), frame token c:  c == e: no candidates (ASG emits a repeated letter through a replabel).  From the empty prefix
 *     a = lp[c], no add and no transition.  Otherwise a = (p + A[c][e]) + lp[c].  The siblings' terms are then added to a in their
 *     order: p' = a + g with a token LM (g as in w2l_ctc_beam_search_lm); in the lexicon search the sil / in / word slots of
 *     w2l_ctc_beam_search_lex with (lp[c] + base) replaced by a.  The transition term is there from an entry's second label on,
 *     which under threshold pruning is not "from frame 1 on"; this is the rule that equals Viterbi.
 *   lm == NULL (w2l_asg_beam_search only): no LM.  No g term is added, lmScores rows are 0 for live rows and -inf for empty ones,
 *     lmHasEos must be 0 and classScore NULL.
 *   Lexicon.  The c == e rule holds for all three slots.  So a word whose spelling (as packed with replabels) needs one token
 *     twice in a row is unreachable, and a word that starts with the token the previous word ended on needs silence between the
 *     two.  Neither is refused.
 *   Merge, prune, order, end (root only, EOS term, re-rank) and outputs are the siblings'.
 * Consequences: with trans = 0 and normalize = 0, labels, lengths and scores equal the CTC sibling's on the same emissions with a
 * column of -inf appended as blank, bit for bit in both logAdd modes; with logAdd = 0, no LM and a beam that never cuts, the
 * 1-best is w2l_viterbi_compute's path collapsed over runs and its score, accumulated in the recursion's order.
 * With logAdd = 0 the result is reproducible bit for bit, ties included (same exception for the sign of a zero).
 * Limits and refusals: the siblings' (N >= 2 kept for uniformity), and trans NULL (W2L_EINVAL), all before anything touches the
 * device.  trans, like lm, lexicon and classScore, is device memory and NOT checked. */
size_t w2l_asg_beam_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_asg_beam_search(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                        const float* trans /*[N][N], to x from, device*/, int beam /*W*/, int beamToken /*K*/, float threshold,
                        int logAdd, int normalize, int nbest /*M*/, int maxLen /*Lmax*/, const void* lm /*or NULL*/, int lmHasEos,
                        float lmWeight, const float* classScore /*[N] or NULL*/, float eosScore,
                        int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                        float* lmScores /*[B][M]*/, void* workspace, w2l_stream_t stream);
size_t w2l_asg_beam_lex_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_asg_beam_search_lex(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                            const float* trans /*[N][N], to x from, device*/, int beam /*W*/, int beamToken /*K*/, float threshold,
                            int logAdd, int normalize, int nbest /*M*/, int maxLen /*Lmax*/, const void* lm, int lmHasEos,
                            float lmWeight, const void* lexicon, float wordScore, float eosScore,
                            int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                            float* lmScores /*[B][M]*/, int maxWords, int* words /*[B][M][maxWords]*/, int* wordCounts /*[B][M]*/,
                            void* workspace, w2l_stream_t stream);
/* The wide twins of the five beam searches above.  Each takes the argument list of its sibling and obeys its sibling's contract
 * word for word -- frame tokens, stay / ext / merge / prune, the order and its tie key, the sil / in / word slots, the ASG rules,
 * the end rule and the EOS term, the outputs, the order of the refusals -- with two differences: W may be 1..1024 and M 1..W.  K
 * after clipping stays <= 64; W > 1024 or K > 64 is W2L_EUNSUPPORTED (and a workspace size of 0), after every W2L_EINVAL, before
 * anything touches the device.  The kernels are another family (one workgroup per utterance, the candidates of a frame in the
 * workspace, a parallel selection of the W best keys and a sort of the survivors), but every value is made by the sibling's
 * operation sequence and the ranks depend on the keys alone: with logAdd = 0 the outputs equal the sibling's bit for bit at every
 * W both accept, and with logAdd = 1 too (a stay receives at most one merged term, so no sum depends on an order).  The workspace
 * grows with W * K (* 7 with a lexicon): 8 bytes per possible candidate of a frame and utterance. */
size_t w2l_ctc_beam_wide_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_wide(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                             int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                             int nbest /*M*/, int maxLen /*Lmax*/,
                             int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                             void* workspace, w2l_stream_t stream);
size_t w2l_ctc_beam_lm_wide_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_lm_wide(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                                int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                                int nbest /*M*/, int maxLen /*Lmax*/, const void* lm, int lmHasEos, float lmWeight,
                                const float* classScore /*[N-1] or NULL*/, float eosScore,
                                int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                                float* lmScores /*[B][M]*/, void* workspace, w2l_stream_t stream);
size_t w2l_ctc_beam_lex_wide_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_lex_wide(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                                 int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                                 int nbest /*M*/, int maxLen /*Lmax*/, const void* lm, int lmHasEos, float lmWeight,
                                 const void* lexicon, float wordScore, float eosScore,
                                 int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                                 float* lmScores /*[B][M]*/, int maxWords, int* words /*[B][M][maxWords]*/,
                                 int* wordCounts /*[B][M]*/, void* workspace, w2l_stream_t stream);
size_t w2l_asg_beam_wide_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_asg_beam_search_wide(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                             const float* trans /*[N][N], to x from, device*/, int beam /*W*/, int beamToken /*K*/, float threshold,
                             int logAdd, int normalize, int nbest /*M*/, int maxLen /*Lmax*/, const void* lm /*or NULL*/,
                             int lmHasEos, float lmWeight, const float* classScore /*[N] or NULL*/, float eosScore,
                             int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                             float* lmScores /*[B][M]*/, void* workspace, w2l_stream_t stream);
size_t w2l_asg_beam_lex_wide_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_asg_beam_search_lex_wide(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                                 const float* trans /*[N][N], to x from, device*/, int beam /*W*/, int beamToken /*K*/,
                                 float threshold, int logAdd, int normalize, int nbest /*M*/, int maxLen /*Lmax*/, const void* lm,
                                 int lmHasEos, float lmWeight, const void* lexicon, float wordScore, float eosScore,
                                 int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                                 float* lmScores /*[B][M]*/, int maxWords, int* words /*[B][M][maxWords]*/,
                                 int* wordCounts /*[B][M]*/, void* workspace, w2l_stream_t stream);
/* The xl twins of the five beam searches: the beam widths the reference's recipes ask for (1500, 2500, 5000, 8000).  Each takes the
 * argument list of its sibling and obeys its sibling's contract word for word -- frame tokens, stay / ext / merge / prune, the order
 * and its tie key, the sil / in / word slots, the ASG rules, the end rule and the EOS term, the outputs, the order of the refusals
 * -- with two differences: W may be 1..8192 and M 1..W.  K after clipping stays <= 64; W > 8192 or K > 64 is W2L_EUNSUPPORTED (and
 * a workspace size of 0), after every W2L_EINVAL, before anything touches the device; T * W > 2^29 is W2L_EUNSUPPORTED as well
 * (node ids are ints).  The kernels are a third family (csrc/criterion_beam_xl.hpp, DESIGN 3.24: the wide family's algorithm with
 * one workgroup per utterance whose threads own entries tid, tid + 1024, ..., the beam, the gone masks and the stays in the
 * workspace, the node -> rank hash and then the survivors' sort in up to 128 KiB of LDS), but every value is made by the sibling's
 * operation sequence and the ranks depend on the keys alone: with logAdd = 0 the outputs equal the wide twin's bit for bit at every
 * W both accept, and with logAdd = 1 they equal them too (a stay receives at most one merged term, so no sum depends on an order).
 * The workspace is the wide twin's at that W -- 8 bytes per possible candidate of a frame and utterance, W * K (* 7 with a
 * lexicon) + W of them -- plus 80 (lexicon: 136) bytes per beam entry and utterance; the prefix table is 8 * pow2(2 * T * W) bytes
 * per utterance, 256 MiB at T = 2000, W = 8192. */
size_t w2l_ctc_beam_xl_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_xl(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                           int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                           int nbest /*M*/, int maxLen /*Lmax*/,
                           int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                           void* workspace, w2l_stream_t stream);
size_t w2l_ctc_beam_lm_xl_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_lm_xl(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                              int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                              int nbest /*M*/, int maxLen /*Lmax*/, const void* lm, int lmHasEos, float lmWeight,
                              const float* classScore /*[N-1] or NULL*/, float eosScore,
                              int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                              float* lmScores /*[B][M]*/, void* workspace, w2l_stream_t stream);
size_t w2l_ctc_beam_lex_xl_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_lex_xl(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                               int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                               int nbest /*M*/, int maxLen /*Lmax*/, const void* lm, int lmHasEos, float lmWeight,
                               const void* lexicon, float wordScore, float eosScore,
                               int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                               float* lmScores /*[B][M]*/, int maxWords, int* words /*[B][M][maxWords]*/,
                               int* wordCounts /*[B][M]*/, void* workspace, w2l_stream_t stream);
size_t w2l_asg_beam_xl_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_asg_beam_search_xl(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                           const float* trans /*[N][N], to x from, device*/, int beam /*W*/, int beamToken /*K*/, float threshold,
                           int logAdd, int normalize, int nbest /*M*/, int maxLen /*Lmax*/, const void* lm /*or NULL*/,
                           int lmHasEos, float lmWeight, const float* classScore /*[N] or NULL*/, float eosScore,
                           int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                           float* lmScores /*[B][M]*/, void* workspace, w2l_stream_t stream);
size_t w2l_asg_beam_lex_xl_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_asg_beam_search_lex_xl(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                               const float* trans /*[N][N], to x from, device*/, int beam /*W*/, int beamToken /*K*/,
                               float threshold, int logAdd, int normalize, int nbest /*M*/, int maxLen /*Lmax*/, const void* lm,
                               int lmHasEos, float lmWeight, const void* lexicon, float wordScore, float eosScore,
                               int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                               float* lmScores /*[B][M]*/, int maxWords, int* words /*[B][M][maxWords]*/,
                               int* wordCounts /*[B][M]*/, void* workspace, w2l_stream_t stream);
/* The five beam searches with a SILENCE SCORE (the reference's --silscore, older name --silweight; csrc/criterion_beam_entry.hpp,
 * DESIGN 3.26).  Each takes `family` first -- 0: the narrow search above, 1: its wide twin, 2: its xl twin --, then its sibling's
 * argument list, then silToken and silScore.  One rule covers all five searches in all three families:
 *   With silToken in range and silScore finite, the frame score of class silToken is replaced, AFTER THE FRAME TOKENS HAVE BEEN
 *   CHOSEN, by lp_t[sil] + silScore: one fp32 add; with normalize = 1 it is (x - lse) + silScore, lse taken from the raw row.
 *   Every later use of lp_t[sil] reads this value: the stay of an entry whose last label is sil; every extension by sil, in the
 *   lexicon searches the root's sil slot and any trie edge on that token; the merged term, thresholds, totals, keys.  Frame
 *   tokens, their order and the tie key's k are still those of the acoustic lp alone: the reference too picks its beamSizeToken
 *   candidates before it adds silScore.
 * Everything else of each sibling's contract is unchanged.  This is the project's own operation sequence: the reference adds the
 * term after the acoustic sum, in double; here it is part of the frame score, in fp32, before any sum.
 * Consequences.  silScore == 0 or silToken == -1: the sibling's call -- the host routes it there, the same kernels and bytes, no
 * + 0 is executed.  normalize = 0 and K >= the token count (selection cannot differ): every output equals, bit for bit, the
 * sibling's on emissions whose sil column had silScore added on the host in fp32, in both logAdd modes; so the ASG max search
 * without LM is still w2l_viterbi_compute's path and score on those emissions.  The three families agree bit for bit at every W two
 * of them accept.
 * The narrow LM-free CTC search with a silence score does not run its sibling's one-wavefront scan, which relies on lp_k + tot
 * being non-increasing in k; it runs the workgroup token scan without an LM, and its workspace is the LM search's.
 * In the lexicon searches silToken is an argument like any other: the caller passes the lexicon's; the blob on the device is not
 * checked against it.
 * Limits and refusals: the chosen family's, in the sibling's order, and before them, before anything touches the device,
 * W2L_EINVAL for family outside 0..2, for silScore not finite, and for silToken outside -1 .. N-2 (CTC: blank is no token) or
 * -1 .. N-1 (ASG).  The *_sil_workspace_size functions are host arithmetic and return 0 for what the call refuses (they do not see
 * silToken and silScore). */
size_t w2l_ctc_beam_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_sil(int family, int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                            int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                            int nbest /*M*/, int maxLen /*Lmax*/,
                            int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                            void* workspace, w2l_stream_t stream, int silToken, float silScore);
size_t w2l_ctc_beam_lm_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_lm_sil(int family, int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                               int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                               int nbest /*M*/, int maxLen /*Lmax*/, const void* lm, int lmHasEos, float lmWeight,
                               const float* classScore /*[N-1] or NULL*/, float eosScore,
                               int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                               float* lmScores /*[B][M]*/, void* workspace, w2l_stream_t stream, int silToken, float silScore);
size_t w2l_ctc_beam_lex_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_lex_sil(int family, int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                                int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                                int nbest /*M*/, int maxLen /*Lmax*/, const void* lm, int lmHasEos, float lmWeight,
                                const void* lexicon, float wordScore, float eosScore,
                                int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                                float* lmScores /*[B][M]*/, int maxWords, int* words /*[B][M][maxWords]*/,
                                int* wordCounts /*[B][M]*/, void* workspace, w2l_stream_t stream, int silToken, float silScore);
size_t w2l_asg_beam_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken);
int w2l_asg_beam_search_sil(int family, int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                            const float* trans /*[N][N], to x from, device*/, int beam /*W*/, int beamToken /*K*/, float threshold,
                            int logAdd, int normalize, int nbest /*M*/, int maxLen /*Lmax*/, const void* lm /*or NULL*/,
                            int lmHasEos, float lmWeight, const float* classScore /*[N] or NULL*/, float eosScore,
                            int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                            float* lmScores /*[B][M]*/, void* workspace, w2l_stream_t stream, int silToken, float silScore);
size_t w2l_asg_beam_lex_sil_workspace_size(int family, int B, int T, int N, int beam, int beamToken);
int w2l_asg_beam_search_lex_sil(int family, int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                                const float* trans /*[N][N], to x from, device*/, int beam /*W*/, int beamToken /*K*/,
                                float threshold, int logAdd, int normalize, int nbest /*M*/, int maxLen /*Lmax*/, const void* lm,
                                int lmHasEos, float lmWeight, const void* lexicon, float wordScore, float eosScore,
                                int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                                float* lmScores /*[B][M]*/, int maxWords, int* words /*[B][M][maxWords]*/,
                                int* wordCounts /*[B][M]*/, void* workspace, w2l_stream_t stream, int silToken, float silScore);
/* The MANY-TOKEN twins of the five beam searches (the reference's --beamsizetoken above 64: 100 in its word-piece recipes, 150;
 * csrc/criterion_beam_xl.hpp).  Each takes its xl twin's argument list, then silToken and silScore, and obeys the
 * sibling's contract word for word -- the frame tokens are the K best non-blank classes by lp descending, class ascending; stay /
 * ext / merge / prune; the order total descending, rank ascending, stay before extension, k ascending, slot ascending; the
 * threshold line, the lexicon slots, the ASG rules, the end rule and the EOS term; the silence rule of the *_sil entry points
 * (tokens are chosen by the acoustic lp alone, then lp[sil] + silScore is read wherever the search reads it); the outputs -- with
 * one difference: W may be 1..8192 as in the xl twins and K AFTER CLIPPING MAY BE 1..256.  silToken = -1 or silScore == 0: no
 * silence score, and no + 0 is executed.
 * Consequences.  At K <= 64 every output equals the xl twin's bit for bit (with a silence score: the *_sil entry point's at
 * family 2), in both logAdd modes; nothing is routed there, the many-token kernels run.
 * The kernels are the xl family's scan with what a token count above 64 touches changed: 256 LDS slots of frame tokens, gone masks
 * of ceil(K / 64) 64-bit words per (slot, entry) in the workspace (word k >> 6, bit k & 63), a tie key with 8 bits of k
 * (r << 12 | ext << 11 | k << 3 | slot: the same lexicographic order, so the same ranks), and a candidate list of W * K (* 7 with
 * a lexicon) + W keys counted in size_t.  The row pass and the finish are the xl twins'.
 * Refusals, in the xl twin's order, before anything touches the device: its W2L_EINVALs and those of the *_sil entry points
 * (silScore not finite; silToken outside -1 .. N-2 for CTC, -1 .. N-1 for ASG); then W2L_EUNSUPPORTED for W > 8192, for K > 256
 * after clipping, and for T * W > 2^29.  The *_mt_workspace_size functions are host arithmetic and return 0 for what the call
 * refuses; at K <= 64 the size is the xl twin's, above it the candidate list grows with K and the masks by 8 bytes per (slot,
 * entry) and further word: 8192 * 256 * 7 + 8192 keys are 112 MiB per utterance.
 * Only these ten entry points take K above 64.  The narrow, wide and xl searches, the *_sil and *_lextok entry points and the beam
 * sessions keep K <= 64 and their refusals. */
size_t w2l_ctc_beam_mt_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_mt(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                           int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                           int nbest /*M*/, int maxLen /*Lmax*/,
                           int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                           void* workspace, w2l_stream_t stream, int silToken, float silScore);
size_t w2l_ctc_beam_lm_mt_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_lm_mt(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                              int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                              int nbest /*M*/, int maxLen /*Lmax*/, const void* lm, int lmHasEos, float lmWeight,
                              const float* classScore /*[N-1] or NULL*/, float eosScore,
                              int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                              float* lmScores /*[B][M]*/, void* workspace, w2l_stream_t stream, int silToken, float silScore);
size_t w2l_ctc_beam_lex_mt_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_lex_mt(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                               int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                               int nbest /*M*/, int maxLen /*Lmax*/, const void* lm, int lmHasEos, float lmWeight,
                               const void* lexicon, float wordScore, float eosScore,
                               int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                               float* lmScores /*[B][M]*/, int maxWords, int* words /*[B][M][maxWords]*/,
                               int* wordCounts /*[B][M]*/, void* workspace, w2l_stream_t stream, int silToken, float silScore);
size_t w2l_asg_beam_mt_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_asg_beam_search_mt(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                           const float* trans /*[N][N], to x from, device*/, int beam /*W*/, int beamToken /*K*/, float threshold,
                           int logAdd, int normalize, int nbest /*M*/, int maxLen /*Lmax*/, const void* lm /*or NULL*/,
                           int lmHasEos, float lmWeight, const float* classScore /*[N] or NULL*/, float eosScore,
                           int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                           float* lmScores /*[B][M]*/, void* workspace, w2l_stream_t stream, int silToken, float silScore);
size_t w2l_asg_beam_lex_mt_workspace_size(int B, int T, int N, int beam, int beamToken);
int w2l_asg_beam_search_lex_mt(int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                               const float* trans /*[N][N], to x from, device*/, int beam /*W*/, int beamToken /*K*/,
                               float threshold, int logAdd, int normalize, int nbest /*M*/, int maxLen /*Lmax*/, const void* lm,
                               int lmHasEos, float lmWeight, const void* lexicon, float wordScore, float eosScore,
                               int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                               float* lmScores /*[B][M]*/, int maxWords, int* words /*[B][M][maxWords]*/,
                               int* wordCounts /*[B][M]*/, void* workspace, w2l_stream_t stream, int silToken, float silScore);
/* The lexicon searches with a TOKEN-LEVEL LM (the reference's --uselexicon=true --decodertype=tkn; csrc/criterion_beam_lextok.hpp,
 * DESIGN 3.27): the lexicon constrains the spellings, the LM scores the tokens.  The argument lists are those of
 * w2l_ctc_beam_search_lex_sil and w2l_asg_beam_search_lex_sil, and the contract is w2l_ctc_beam_search_lex's (ASG:
 * w2l_asg_beam_search_lex's) with these changes.
 * `lm` is a w2l_ngram_lm_* blob over the lexicon's numTokens TOKENS, not over its words; EOS is word numTokens + 1.
 * State: unchanged -- e, pb, pnb, lexicon node u, LM state s, word list, the unweighted LM sum acc.  The trie's smear values are
 * never read: a smeared and an unsmeared blob give the same bytes.
 * Extensions of entry r by frame token c, base = (c == e ? pb : tot):
 *   sil, slot 0     c == silToken (the lexicon's) and u the root: as in the sibling.  pnb' = lp[c] + base, the state stays s, no LM
 *                   term, acc unchanged.
 *   otherwise       v = child(u, c); without a child there are no candidates.  a = (lp[c] + base) + (lmWeight * q(s, c)): one fp32
 *                   multiply, then one add to the acoustic sum.  s' is q's successor, acc' = acc + q.  A trie edge on the silence
 *                   token inside a spelling is a token like any other and is LM-scored.
 *   in, slot 0      v has children: pnb' = a; the new entry is at v with state s'.
 *   word i, 1 + i   pnb' = a + wordScore, one add; the new entry is at the root with state s', w is appended.  Homophones tie and
 *                   are ordered by slot.
 * One LM lookup per (entry, token) pair.  ASG: (lp[c] + base) is the policy's a, (tot + A[c][e]) + lp[c], and c == e has no
 * candidates in any slot.  Merge, prune, order (total, r, stay first, k, slot), end (root only; the EOS term lmWeight * q(s, EOS) +
 * eosScore from the token LM; re-rank), outputs and lmScores keep the sibling's rules.  The silence score: the rule of the *_sil
 * entry points above; silScore == 0 or silToken == -1 means none, and no + 0 is executed.
 * Consequences.  With a lexicon that holds every token as a one-token word, no silence token, wordScore = 0: labels, lengths,
 * scores and lmScores are w2l_ctc_beam_search_lm's (w2l_asg_beam_search's) with classScore = NULL, bit for bit.  With
 * lmWeight = 0 and lmHasEos = 0: everything but lmScores is w2l_*_beam_search_lex's on an unsmeared lexicon, bit for bit.
 * Not part of the contract: an unknown-word arc, log-add smearing, LM orders above the blob format's 8.
 * family: 0 narrow (W <= 64), 1 wide (W <= 1024); the two agree bit for bit at W <= 64.  family 2 (xl) is W2L_EUNSUPPORTED and its
 * workspace size is 0.  Refusals, all before anything touches the device: W2L_EINVAL for family outside 0..2, silScore not finite,
 * silToken out of range (as above); W2L_EUNSUPPORTED for family 2; then the chosen family's lexicon search's, in its order.  The
 * workspace is the lexicon search's of that family. */
size_t w2l_ctc_beam_lextok_workspace_size(int family, int B, int T, int N, int beam, int beamToken);
int w2l_ctc_beam_search_lextok(int family, int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                               int beam /*W*/, int beamToken /*K*/, float threshold, int logAdd, int normalize,
                               int nbest /*M*/, int maxLen /*Lmax*/, const void* lm /*over tokens*/, int lmHasEos, float lmWeight,
                               const void* lexicon, float wordScore, float eosScore,
                               int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                               float* lmScores /*[B][M]*/, int maxWords, int* words /*[B][M][maxWords]*/,
                               int* wordCounts /*[B][M]*/, void* workspace, w2l_stream_t stream, int silToken, float silScore);
size_t w2l_asg_beam_lextok_workspace_size(int family, int B, int T, int N, int beam, int beamToken);
int w2l_asg_beam_search_lextok(int family, int B, int T, int N, const float* input /*[B][T][N]*/, const int* frames /*[B] or NULL*/,
                               const float* trans /*[N][N], to x from, device*/, int beam /*W*/, int beamToken /*K*/,
                               float threshold, int logAdd, int normalize, int nbest /*M*/, int maxLen /*Lmax*/,
                               const void* lm /*over tokens*/, int lmHasEos, float lmWeight, const void* lexicon, float wordScore,
                               float eosScore, int* labels /*[B][M][Lmax]*/, int* lengths /*[B][M]*/, float* scores /*[B][M]*/,
                               float* lmScores /*[B][M]*/, int maxWords, int* words /*[B][M][maxWords]*/,
                               int* wordCounts /*[B][M]*/, void* workspace, w2l_stream_t stream, int silToken, float silScore);

/* ------------------------------------------------------------------------
 * 2. Network operators (fp32).  Activations are FRAME-MAJOR: a tensor the
 * reference holds as ArrayFire dims (T, H, C, B) lives here as x[B][T][H][C]
 * (C fastest), i.e. a row-major [M = B*T*H][C] matrix; Linear layers see
 * [M = B*T][H*C].  Replaces fl::conv2d / fl::linear / fl::LayerNorm /
 * fl::GatedLinearUnit / fl::Dropout autograd functions (un-vendored Flashlight;
 * grammar in recipes/joint_training_vox_populi/cpc/SequentialBuilder.cpp:92-626).
 * ---------------------------------------------------------------------- */

/* generic C[M][N] = op(A) op(B) (+bias[n]) (relu). a_kcontig: A stored [M][K];
 * else [K][M]. b_kcontig: B stored [N][K]; else [K][N]. splitk > 1: atomics. */
int w2l_gemm_f32(int M, int N, int K, const float* A, int lda, int a_kcontig, const float* B,
                 int ldb, int b_kcontig, float* C, int ldc, const float* bias, int relu,
                 int splitk, w2l_stream_t stream);

/* fl::Linear: y[M][out] = x[M][in] . w[in][out] + bias (w is Flashlight's (out,in)
 * column-major weight, byte-identical); optional fused ReLU. */
int w2l_linear_forward(int M, int in, int out, const float* x, const float* w,
                       const float* bias, float* y, int relu, w2l_stream_t stream);
int w2l_linear_backward_data(int M, int in, int out, const float* dy, const float* w, float* dx,
                             int accumulate, const float* maskSrc, float maskScale,
                             w2l_stream_t stream);
int w2l_linear_backward_weight(int M, int in, int out, const float* x, const float* dy, float* dw,
                               w2l_stream_t stream);
/* both parameter gradients of fl::Linear in one call: dw[in][out] = x^T dy and db[out] = sum_m dy[m][.] (db may be NULL: the
 * call above).  Where the product runs on the 160-wide LDS-DMA kernel the column sums ride on it -- the first tile row adds
 * up the dy fragments it multiplies, no second pass over dy --, otherwise w2l_colsum follows.  Both are deterministic. */
int w2l_linear_backward_weight_bias(int M, int in, int out, const float* x, const float* dy, float* dw, float* db,
                                    w2l_stream_t stream);
/* y = dropout(relu?(x w + b)): fl::Dropout behind a Linear(+ReLU) folded into the GEMM epilogue; bit-identical to
 * w2l_linear_forward followed by w2l_dropout_inplace(y, M*out, p, seed, rngStream) */
/* y = dropout(relu?(x w + b)) + add: the residual join behind a Linear in the same epilogue (fl::TDSBlock: r2 = dropout(lin2) + y1);
 * bit-identical to w2l_linear_forward_dropout followed by an elementwise add of `add` ([M][out]); p = 0: no dropout */
int w2l_linear_forward_dropout_add(int M, int in, int out, const float* x, const float* w, const float* bias, const float* add,
                                   float* y, int relu, double p, uint32_t seed, uint32_t rngStream, w2l_stream_t stream);
int w2l_linear_forward_dropout(int M, int in, int out, const float* x, const float* w, const float* bias,
                               float* y, int relu, double p, uint32_t seed, uint32_t rngStream,
                               w2l_stream_t stream);
/* dx = add + dy w^T (add laid out like dx): the residual join of a backward pass without copying add into dx first */
int w2l_linear_backward_data_add(int M, int in, int out, const float* dy, const float* w, const float* add,
                                 float* dx, w2l_stream_t stream);
/* Mixed precision (BASELINE config 3; fl's --fl_amp_use_mixed_precision, recipes/joint_training_vox_populi/cpc/Train.cpp:1184
 * keeps the criterion input in f32): mode 1 = every fl::Linear GEMM multiplies in bf16 (v_mfma_f32_32x32x16_bf16, operands
 * rounded to nearest even on the way into LDS) and accumulates in fp32; operands, results, master weights and the
 * criteria stay fp32.  Process-wide, returns the previous mode. */
int w2l_set_matmul_precision(int mode);
/* Mixed precision with bf16 OPERAND STORAGE (round 3): the activations, the output gradients and per-step copies of the fp32
 * master weights are kept as bf16 images in HBM and multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; results,
 * bias, every non-GEMM operator and the criterion stay fp32 (cpc/Train.cpp:1184).
 * w2l_bf16_convert: x [rows][cols] fp32 (leading dimension ldx) -> rowMajor [rows][ldRows] and / or transposed [cols][ldTrans]
 *   bf16 (round to nearest even), zero-padded to the leading dimension; either may be NULL; ldRows >= cols, ldTrans >= rows,
 *   both multiples of 16 elements (use the reduction length rounded up to 64); 16-byte aligned outputs.
 * w2l_gemm_bf16: C[M][N] (fp32, ldc) = A[M][K] . B[N][K]^T (+ bias[n]) (ReLU) (dropout) (mask) (+ addend | + C); A and B are
 *   k-contiguous bf16 images whose rows are ZERO from column K up to K rounded to 64 (lda, ldb >= that, even). */
typedef struct {
  const float* mask;  /* v = mask[m][n] > 0 ? v * maskScale : 0  (layout of C) */
  float maskScale;
  const float* addend; /* v += addend[m][n] (layout of C) */
  int accumulate;      /* v += C[m][n] (ignored when addend is set) */
  double dropP;        /* > 0: dropout with the library's stateless hash of (m * ldc + n, dropSeed, dropStream) */
  uint32_t dropSeed, dropStream;
} w2l_gemm_epilogue;
int w2l_bf16_convert(const float* x, size_t rows, int cols, size_t ldx, uint16_t* rowMajor, size_t ldRows,
                     uint16_t* transposed, size_t ldTrans, w2l_stream_t stream);
/* the images of dropout(x): mask and scale of w2l_dropout_copy(p, seed, rngStream) over the dense [rows][ldx] matrix, applied on the
 * way (the masked copy is never written) -- a dropout layer's backward pass when the masked gradient is only a GEMM operand */
int w2l_bf16_convert_dropout(const float* x, size_t rows, int cols, size_t ldx, uint16_t* rowMajor, size_t ldRows,
                             uint16_t* transposed, size_t ldTrans, double p, uint32_t seed, uint32_t rngStream, w2l_stream_t stream);
/* n (1 .. 8) conversions in one launch (small matrices are launch-bound one at a time); each entry = the arguments of w2l_bf16_convert */
typedef struct {
  const float* x;
  size_t rows;
  int cols;
  size_t ldx;
  uint16_t* rowMajor;
  size_t ldRows;
  uint16_t* transposed;
  size_t ldTrans;
} w2l_bf16_convert_desc;
int w2l_bf16_convert_multi(int n, const w2l_bf16_convert_desc* descs, w2l_stream_t stream);
int w2l_gemm_bf16(int M, int N, int K, const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc,
                  const float* bias, int relu, const w2l_gemm_epilogue* epilogue, w2l_stream_t stream);
/* `groups` (1 .. 4) products of ONE shape in one launch, C_g [M][N] = A_g . B_g^T (+ bias_g): the tiles of all problems share the
 * persistent grid (a Transformer block's four C x C weight gradients at M = 3008 frames are 64 tiles each -- a quarter of the chip
 * one at a time).  A, B, C, bias are HOST arrays of device pointers (bias, or single entries of it, may be NULL). */
/* the same with k-MAJOR operands read in place: aKMajor -> A stored [K][lda] (lda >= M), bKMajor -> B stored [K][ldb] (ldb >= N);
 * lda / ldb multiples of 8, bases 16-byte aligned; rows k >= K are not read.  x^T dy from the row-major images of x and dy,
 * x w from the row-major image of w: no transposed bf16 image of either operand */
int w2l_gemm_bf16_ex(int M, int N, int K, const uint16_t* A, int lda, int aKMajor, const uint16_t* B, int ldb, int bKMajor, float* C,
                     int ldc, const float* bias, int relu, const w2l_gemm_epilogue* e, w2l_stream_t stream);
int w2l_gemm_bf16_grouped(int groups, int M, int N, int K, const uint16_t* const* A, int lda, const uint16_t* const* B, int ldb,
                          float* const* C, int ldc, const float* const* bias, w2l_stream_t stream);
int w2l_colsum(const float* x, float* out, size_t M, int N, w2l_stream_t stream); /* bias grads */

/* fl::Conv2D kw x 1 over time (arch tokens C / C2 / TDS). x [B][T][H][Cin],
 * w [kw][Cin][Cout], y [B][To][H][Cout]; cross-correlation, zero padding. */
typedef struct {
  int B, T, H, Cin, Cout, kw, stride, padl, padr;
} w2l_conv_desc;
int w2l_conv_out_len(int T, int kw, int stride, int padl, int padr);
int w2l_conv_same_pad(int T, int kw, int stride); /* PaddingMode::SAME (pad = -1) */
int w2l_conv_forward(const w2l_conv_desc* d, const float* x, const float* w, const float* bias,
                     float* y, int relu, w2l_stream_t stream);
int w2l_conv_backward_data(const w2l_conv_desc* d, const float* dy, const float* w, float* dx,
                           int accumulate, w2l_stream_t stream);
/* dx = add + backward-data(dy, w): fused residual join (add has the layout of dx) */
int w2l_conv_backward_data_add(const w2l_conv_desc* d, const float* dy, const float* w,
                               const float* add, float* dx, w2l_stream_t stream);
int w2l_conv_backward_filter(const w2l_conv_desc* d, const float* x, const float* dy, float* dw,
                             float* dbias, w2l_stream_t stream);
/* The kw x 1 convolutions over the mel rows of the TDS recipes in the mixed-precision mode (bf16 operand storage, see
 * w2l_gemm_bf16) -- fl::TDSBlock's time convolution (C -> C channels, stride 1) and the sub-sampling `C2 cin cout kw 1 s 1`
 * lines between the blocks (cin != cout <= 32 channels, stride 1 or 2, any padding): x / dy and the weights rounded to bf16,
 * fp32 accumulation on v_mfma_f32_32x32x16_bf16, fp32 bias / ReLU / addend / results (conv_tds_bf16.hip).  Layouts as
 * w2l_conv_*: x [B][T][H][Cin], w [kw][Cin][Cout], y / dy [B][To][H][Cout].
 * w2l_tds_conv_bf16_image_elems: bf16 elements of ONE weight image buffer of the geometry (the forward image, or the images
 *   of all phases of a strided backward-data pass, whichever is larger); 0 = no bf16 kernel for it (use w2l_conv_*).
 * w2l_tds_conv_bf16_prepare: once per step, the forward and the backward-data images of the fp32 weights.
 * backward_filter: dw only (H % 16 == 0); backward_filter_bias: dw and the bias gradient (sums of the ROUNDED dy) in one launch. */
size_t w2l_tds_conv_bf16_image_elems(const w2l_conv_desc* d);
int w2l_tds_conv_bf16_prepare(const w2l_conv_desc* d, const float* w, uint16_t* imgForward, uint16_t* imgBackward, w2l_stream_t stream);
int w2l_tds_conv_bf16_forward(const w2l_conv_desc* d, const float* x, const uint16_t* imgForward, const float* bias, float* y,
                              int relu, w2l_stream_t stream);
int w2l_tds_conv_bf16_backward_data(const w2l_conv_desc* d, const float* dy, const uint16_t* imgBackward, const float* add,
                                    float* dx, w2l_stream_t stream);
int w2l_tds_conv_bf16_backward_filter(const w2l_conv_desc* d, const float* x, const float* dy, float* dw, w2l_stream_t stream);
/* the same launch also produces dbias [Cout] = column sums of the bf16-rounded dy (summed from the slabs the kernel stages anyway) */
int w2l_tds_conv_bf16_backward_filter_bias(const w2l_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                                           w2l_stream_t stream);
/* The WIDE time convolution at H == 1 in the mixed-precision mode (conv_bf16.hip): the `C cin cout kw s pad` lines of the conv_glu
 * recipes, the lexicon-free recipe and the Transformer recipes' front end.  Same contract as the TDS family above -- x / dy and w
 * rounded to bf16 (nearest even), v_mfma_f32_32x32x16_bf16 products, fp32 accumulation / bias / ReLU / addend / results, dbias =
 * column sums of the ROUNDED dy, run-to-run deterministic -- and the layouts of w2l_conv_*.  Accepted: H == 1, stride 1 or 2,
 * 32 <= Cin <= 8192 and Cout <= 8192 (any value, multiples of 8 or not), kw <= 64, any padl / padr >= 0, any T with To >= 1, every
 * operand image below 2 GiB.  Anything else: both size queries return 0 and the calls W2L_EUNSUPPORTED (stay on w2l_conv_*).
 * Null pointers, misaligned images and bad descriptors: W2L_EINVAL.  All checks precede the first launch; the size queries are
 * host arithmetic.
 * w2l_conv_bf16_image_elems: bf16 elements of ONE weight image buffer (two are needed: forward, backward-data).
 * w2l_conv_bf16_scratch_elems: bf16 elements of the caller-owned scratch the passes write the activation / gradient images to
 *   (16-byte aligned; nothing in it outlives a call, so one buffer may serve every layer of a network on one stream).
 * w2l_conv_bf16_prepare: once per step, the two images of the fp32 weight (either pointer may be NULL). */
size_t w2l_conv_bf16_image_elems(const w2l_conv_desc* d);
size_t w2l_conv_bf16_scratch_elems(const w2l_conv_desc* d);
int w2l_conv_bf16_prepare(const w2l_conv_desc* d, const float* w, uint16_t* imgForward, uint16_t* imgBackward, w2l_stream_t stream);
int w2l_conv_bf16_forward(const w2l_conv_desc* d, const float* x, const uint16_t* imgForward, const float* bias, float* y, int relu,
                          uint16_t* scratch, w2l_stream_t stream);
int w2l_conv_bf16_backward_data(const w2l_conv_desc* d, const float* dy, const uint16_t* imgBackward, const float* add, float* dx,
                                uint16_t* scratch, w2l_stream_t stream);
int w2l_conv_bf16_backward_filter_bias(const w2l_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                                       uint16_t* scratch, w2l_stream_t stream);

/* bf16 operand images written by the kernel that PRODUCES a matrix [rows][cols] instead of a w2l_bf16_convert pass over an fp32
 * copy (mixed-precision mode): `rowMajor` [rows][ldRows] and / or `transposed` [cols][ldTrans], the layouts of w2l_bf16_convert;
 * either pointer may be NULL.  Only elements of the matrix are written (a kernel may write zeros into the padding): the zero
 * padding w2l_bf16_convert leaves beyond cols / rows must already be there -- images the caller zero-filled once. */
typedef struct {
  uint16_t* rowMajor;
  size_t ldRows;
  uint16_t* transposed;
  size_t ldTrans;
} w2l_bf16_image_sink;
/* w2l_gemm_bf16 whose RESULT leaves as the bf16 images the next products read (`images`: row-major [M][ldRows] and / or transposed
 * [N][ldTrans], what w2l_bf16_convert would make of C bit for bit; only elements of the matrix are written) instead of, or beside,
 * the fp32 C (C may be NULL when images are given); maskImage: the mask operand as a bf16 row-major image [M][ldMask] (> 0 test,
 * replaces epilogue->mask).  An activation that is only ever a GEMM operand and a ReLU / dropout mask then lives only as bf16,
 * as under the reference's AMP (recipes/slimIPL/src/Train.cpp:209-216).  N % 4 == 0; ldc (>= N) still names the flat index
 * m * ldc + n of the dropout hash.  W2L_EUNSUPPORTED where the wide epilogue cannot run. */
int w2l_gemm_bf16_images(int M, int N, int K, const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc,
                         const float* bias, int relu, const w2l_gemm_epilogue* epilogue, const w2l_bf16_image_sink* images,
                         const uint16_t* maskImage, size_t ldMask, float maskScale, w2l_stream_t stream);
/* w2l_gemm_bf16_smallm (csrc/gemm_smallm.hip): the same product for FEW rows -- the M = slots x a few frames of a streaming step,
 * where the block tiles of w2l_gemm_bf16 leave most of the chip idle.  C[M][N] (fp32, ldc >= N) = A[M][K] . B[N][K]^T (+ bias[n])
 * (ReLU) (+ addend[m][n], the layout of C), bf16 operands, fp32 accumulation.
 *   A: row-major activation image [M][lda], B: transposed weight image [N][ldb], as w2l_bf16_convert writes them: rows ZERO from
 *      column K up to K rounded to 64; lda, ldb >= that and multiples of 8; 16-byte aligned bases.
 *   image: NULL, or a sink whose rowMajor image [M][ldRows >= N] receives what w2l_bf16_convert would make of C, bit for bit (only
 *      elements of the matrix are written); its `transposed` must be NULL (W2L_EINVAL otherwise).  C may be NULL when the image is given.
 *   Any N >= 1 and K >= 1; M from 1 to w2l_gemm_bf16_smallm_max_m() (1024).  Above it: W2L_EUNSUPPORTED -- stay on w2l_gemm_bf16.
 *   workspace: w2l_gemm_bf16_smallm_workspace_bytes(M, N, K) bytes on the device.  The query is host arithmetic and returns 0
 *      today (one launch, no partial sums: pass NULL, 0); query and arguments stay so that a variant that needs one keeps the ABI.
 * Every weight byte is read from HBM once per call, in whole 128-byte lines along K.  K is NOT split: an element is one chain of
 * MFMAs over k = 0, 16, 32, ..., the chain and the epilogue arithmetic of w2l_gemm_bf16 -- wherever that one does not split K
 * itself (K < 4096) the two results are bit-identical, which is what lets a session equal the trainer's forward: any other
 * summation order, however accurate, moves bf16 roundings of the activations and the difference grows block by block (DESIGN
 * 3.14).  Occupancy comes from narrow slabs of weight rows (16; 32 from N = 4096).  The call is deterministic, and row r of the
 * result is a function of row r of A and of B only: bit-identical whatever M is and whatever the other rows of A hold, NaN included.
 * Null pointers, non-positive sizes, a leading dimension below K (rounded to 64): W2L_EINVAL.  All checks precede the first
 * launch.  The probe library returns W2L_EUNSUPPORTED for every call while W2L_SMALLM_OFF is set. */
int w2l_gemm_bf16_smallm_max_m(void);
size_t w2l_gemm_bf16_smallm_workspace_bytes(int M, int N, int K);
int w2l_gemm_bf16_smallm(int M, int N, int K, const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc,
                         const float* bias, int relu, const float* addend, const w2l_bf16_image_sink* image, void* workspace,
                         size_t workspaceBytes, w2l_stream_t stream);
/* r = dropout(a) + x ; y = LayerNorm(r) over `groups` contiguous chunks of `inner`
 * elements with scalar affine gammaBeta[2] (fl::LayerNorm axes {0,1,2}: groups = B).
 * a is updated in place to its dropped value; r, meanRstd[2*groups] are kept for
 * backward; stats / sums are double[w2l_layernorm_scratch_doubles(groups, inner)] scratch
 * (per-block partial sums, added in a fixed order: no atomics, run-to-run deterministic).  Dropout mask = stateless hash of
 * (flat index, seed, rngStream), reproduced bit-exactly by the oracle. */
size_t w2l_layernorm_scratch_doubles(int groups, size_t inner);
int w2l_residual_layernorm_forward(int groups, size_t inner, float* a, const float* x, float* r,
                                   float* y, const float* gammaBeta, float eps, double p,
                                   uint32_t seed, uint32_t rngStream, double* stats,
                                   float* meanRstd, w2l_stream_t stream);
int w2l_layernorm_backward(int groups, size_t inner, const float* r, const float* dy,
                           const float* gammaBeta, const float* meanRstd, float* dr,
                           float* dGammaBeta, const float* maskSrc, float* dmask, float maskScale,
                           double* sums, w2l_stream_t stream);
/* The per-frame LayerNorm of the mixed-precision mode with the images of its result written in the same pass
 * (layernorm_images.hip): as the two calls above for rows of inner <= 2304 floats (inner % 4 == 0; W2L_EUNSUPPORTED otherwise: run
 * the plain call and w2l_bf16_convert), plus yImages = images of y, resp. drImages = images of dr -- of dropout(dr) when
 * imageDropP > 0 (the mask of w2l_dropout_copy with imageDropSeed / imageDropStream over the flat index; dr itself stays
 * unmasked: what w2l_bf16_convert_dropout produced).  ldTrans must hold the rows rounded up to 16 (runs of 16 rows are written).
 * Replaces: fl::LayerNorm + the AMP casts of the next fl::Linear (recipes/slimIPL/src/Train.cpp:209-216). */
int w2l_residual_layernorm_forward_images(int groups, size_t inner, float* a, const float* x, float* r, float* y,
                                          const float* gammaBeta, float eps, double p, uint32_t seed, uint32_t rngStream,
                                          float* meanRstd, const w2l_bf16_image_sink* yImages, w2l_stream_t stream);
int w2l_layernorm_backward_images(int groups, size_t inner, const float* r, const float* dy, const float* gammaBeta,
                                  const float* meanRstd, float* dr, float* dGammaBeta, const float* maskSrc, float* dmask,
                                  float maskScale, double* sums, const w2l_bf16_image_sink* drImages, double imageDropP,
                                  uint32_t imageDropSeed, uint32_t imageDropStream, w2l_stream_t stream);
int w2l_dropout_inplace(float* x, size_t n, double p, uint32_t seed, uint32_t rngStream,
                        w2l_stream_t stream);
/* y = dropout(x) out of place, same mask as w2l_dropout_inplace (16-byte aligned x, y) */
int w2l_dropout_copy(float* y, const float* x, size_t n, double p, uint32_t seed, uint32_t rngStream,
                     w2l_stream_t stream);
int w2l_mask_backward(const float* dy, const float* src, float* dx, size_t n, float scale,
                      w2l_stream_t stream);

/* fl::Conv2D with a kh x kw kernel, kh > 1 (the "C2 cin cout kw kh sx 1 px -1" lines of
 * recipes/sota/2019/am_arch/am_tds_ctc_librivox.arch:3-26; builder recipes/joint_training_vox_populi/cpc/SequentialBuilder.cpp:285-300)
 * runs as a kw x 1 convolution over kh*C channels: xe[r][h][dh*C + c] = x[r][h + dh - padh][c], zero outside the mel
 * axis; rows = utterances x frames.  _backward is the adjoint (sum over dh). */
int w2l_hexpand_forward(const float* x, float* xe, size_t rows, int H, int C, int kh, int padh, w2l_stream_t stream);
int w2l_hexpand_backward(const float* dxe, float* dx, size_t rows, int H, int C, int kh, int padh, w2l_stream_t stream);
/* fl::Transformer's attention core (arch token `TR`, recipes/sota/2019/am_arch/am_transformer_ctc.arch:15-38; block:
 * recipes/joint_training_vox_populi/cpc/TransformerCPC.cpp:117-151; fl::multiheadAttention is [UNVENDORED] Flashlight).
 * Strided batched GEMM over G1 x G2 problems, C = (C +) A B: element (m, k) of A of problem (g1, g2) at
 * A[g1*a1 + g2*a2 + m*sam + k*sak], (k, n) of B at B[g1*b1 + g2*b2 + k*sbk + n*sbn], (m, n) of C at
 * C[g1*c1 + g2*c2 + m*ldc + n]; strides in floats.  With frame-major [B][T][heads*d] q / k / v this is QK^T, PV and their
 * gradients per (utterance, head) without a transpose. */
typedef struct {
  int M, N, K, G1, G2;
  long long sam, sak, a1, a2;
  long long sbk, sbn, b1, b2;
  long long ldc, c1, c2;
  int accumulate;
  /* banded A operand (w2l_bgemm_bf16 only; 0 = dense): the skewed score gradient dR of the relative-position products is non-zero,
   * in row (b, i, h), only at the bandT table rows w = j - i + bandOff, j in [0, bandT).  1: rows = (b, i, h) flattened (bandH heads),
   * k = w; 2: rows = w, k = (i, h) flattened.  K tiles outside the band are skipped (they multiply exact zeros). */
  int bandMode, bandT, bandH, bandOff;
} w2l_bgemm_desc;
int w2l_bgemm_f32(const w2l_bgemm_desc* d, const float* A, const float* B, float* C, w2l_stream_t stream);
/* the same product with bf16 multiplies: fp32 operands rounded to nearest-even bf16 on the way into LDS, v_mfma_f32_32x32x16_bf16,
 * fp32 accumulation and result (BASELINE config 5, "bf16 MFMA attention") */
int w2l_bgemm_bf16(const w2l_bgemm_desc* d, const float* A, const float* B, float* C, w2l_stream_t stream);
/* S[b][h][i][j] (in: q_i . k_j) -> P = softmax_j(scale * (S + R[(b*T + i)*H + h][j - i + n0 - rlo])) in place; R (may be
 * NULL: no position term) holds q_i . E[rlo + w] for w < W, row stride ldr; entries outside [0, W) count as 0
 * (relativePositionEmbeddingRotate pads with zeros).  keyLen (may be NULL): keys j >= keyLen[b] are padding and get
 * probability 0 (the log(padMask) term of TransformerCPC.cpp:138-144). */
int w2l_attn_softmax_forward(float* S, const float* R, const int* keyLen, int B, int H, int T, int ldr, int rlo, int W, int n0,
                             float scale, w2l_stream_t stream);
/* The attention core of one Transformer block's FORWARD pass in one launch (mixed-precision mode; attention_fused.hip):
 *   P = softmax_j(scale * (q_i . k_j + q_i . posTable[j - i + n0]) + log padMask),  Pd = dropout(P),  ctx_i = sum_j Pd[i][j] v_j
 * q, k, v: [B][T][ld] fp32, head h in columns h*d .. (h+1)*d (ld = C, or 3 C for an interleaved q|k|v buffer); posTable: the
 * [2 csz - 1][d] table in the library's internal layout or NULL; rows rlo .. rlo + W are the ones T frames reach (entries outside
 * count as 0); keyLen as in w2l_attn_softmax_forward.  Writes P [B][H][T][T] (the backward pass reads it), Pd (same shape, only when
 * dropP > 0: the same keep pattern as w2l_dropout_copy over P) and ctx [B][T][ldc].  Operands are rounded to bf16 where
 * w2l_bgemm_bf16 rounds them; the result equals the unfused sequence to fp32 summation order.
 * W2L_EUNSUPPORTED when the geometry has no fused kernel (d in {32, 256}, T <= 192, 16-byte aligned rows): run the unfused one.
 * Replaces: TransformerCPC.cpp:117-151 (selfAttention) for the forward pass. */
typedef struct {
  int B, H, T, d;
  int ld, ldc;
  int W, n0, rlo;
  float scale;
  double dropP;
  uint32_t dropSeed, dropStream;
} w2l_attn_fused_desc;
int w2l_attn_fused_forward(const w2l_attn_fused_desc* d, const float* q, const float* k, const float* v, const float* posTable,
                           const int* keyLen, float* P, float* Pd, float* ctx, w2l_stream_t stream);
/* The attention core of the same block's BACKWARD pass (mixed-precision mode; attention_fused_bwd.hip): from dctx [B][T][ldc], the
 * forward's P and its operands
 *   dP = dctx v^T with the forward's dropout mask (recomputed from dropP / dropSeed / dropStream: Pd is not read),
 *   dS = scale * P o (dP - rowsum(P o dP)),   dq_i = sum_j dS[i][j] (k_j + posTable[j - i + n0]),   dk_j = sum_i dS[i][j] q_i,
 *   dv_j = sum_i Pd[i][j] dctx_i,   dPosTable[w] = sum_(b, h, i) dS[i][i + w - n0] q_i
 * in four launches (E^T image, query side, key side, table-gradient reduce) instead of eleven.  dq, dk, dv: [B][T][ld]
 * (overwritten); dPosTable: the whole [2 n0 + 1][d] table gradient (overwritten, zero outside the rows T frames reach; ignored
 * when posTable is NULL).  Operands are rounded to bf16 where the unfused w2l_bgemm_bf16 sequence rounds them (dctx, v, Pd, dS, k,
 * q, posTable); the result equals that sequence to fp32 summation order.  workspace: w2l_attn_fused_backward_workspace(d,
 * posTable != NULL) bytes, 256-byte aligned; it holds the bf16 images dS^T / Pd^T [B H][32 NT][32 NT] (row = key, column = query,
 * NT = ceil(T / 32) rounded up to 2, 4 or 6) first, which tests read.  The key-padding mask needs no argument: P is zero there.
 * W2L_EUNSUPPORTED (workspace size 0) for a geometry without a fused kernel: the same set as the forward call.
 * Replaces: the gradient of TransformerCPC.cpp:117-151 (selfAttention). */
/* The same two calls writing the bf16 images the NEXT product reads (w2l_bf16_image_sink) instead of, or beside, the fp32 result
 * [B T][ldc or ld]: no fp32 copy, no w2l_bf16_convert pass.  The fp32 pointer may be NULL when images are given. */
int w2l_attn_fused_forward_images(const w2l_attn_fused_desc* d, const float* q, const float* k, const float* v, const float* posTable,
                                  const int* keyLen, float* P, float* Pd, float* ctx, const w2l_bf16_image_sink* ctxImages,
                                  w2l_stream_t stream);
int w2l_attn_fused_backward_images(const w2l_attn_fused_desc* d, const float* q, const float* k, const float* v, const float* posTable,
                                   const float* P, const float* dctx, float* dq, float* dk, float* dv,
                                   const w2l_bf16_image_sink* dqImages, const w2l_bf16_image_sink* dkImages,
                                   const w2l_bf16_image_sink* dvImages, float* dPosTable, void* workspace, size_t workspaceBytes,
                                   w2l_stream_t stream);
size_t w2l_attn_fused_backward_workspace(const w2l_attn_fused_desc* d, int withPosTable);
int w2l_attn_fused_backward(const w2l_attn_fused_desc* d, const float* q, const float* k, const float* v, const float* posTable,
                            const float* P, const float* dctx, float* dq, float* dk, float* dv, float* dPosTable, void* workspace,
                            size_t workspaceBytes, w2l_stream_t stream);
/* valid keys per utterance from the batch's input sizes (any unit), as forwardSequentialModuleWithPadMask builds the mask
 * (cpc/SequentialBuilder.cpp:58-81): n_b = ceil(size_b * Tin / max size) valid input frames, resized to Tk (nearest) */
int w2l_attn_key_lengths(const float* inputSizes, int B, int Tin, int Tk, int* keyLen, w2l_stream_t stream);
/* the same for a batch padded BEYOND its longest utterance: *fullSize (device scalar, same unit; NULL = the call above) is the
 * size the Tin input frames correspond to and replaces max size as the denominator */
int w2l_attn_key_lengths_full(const float* inputSizes, const float* fullSize, int B, int Tin, int Tk, int* keyLen,
                              w2l_stream_t stream);
/* dS (in: dL/dP) -> dL/dS (pre-scale scores) in place; dR [B*T*H][ldr] (may be NULL) receives the skewed copy, zeros elsewhere:
 * every column of a row up to ldr is written, so the columns from W to ldr are zero padding that belongs to dR */
int w2l_attn_softmax_backward(const float* P, float* dS, float* dR, int B, int H, int T, int ldr, int rlo, int W, int n0,
                              float scale, w2l_stream_t stream);
/* fl::Pool2D(w, 1, stride, 1, 0, 0, MAX) over time on frame-major x[B][T][F] -> y[B][(T-w)/stride+1][F] (arch token `M`,
 * SequentialBuilder.cpp:398-414); backward routes each dy to the first maximum of its window */
int w2l_pool_time_forward(const float* x, float* y, int B, int T, int F, int w, int stride, w2l_stream_t stream);
int w2l_pool_time_backward(const float* x, const float* dy, float* dx, int B, int T, int F, int w, int stride,
                           w2l_stream_t stream);
int w2l_axpy(float* y, const float* x, size_t n, float alpha, w2l_stream_t stream);
/* The join of a residual block (arch tokens RES / SKIP / SKIPL; [UNVENDORED] fl::Residual: this comment is the contract).
 * forward: y[i] = scale * (a[i] + b[i]) -- one fp32 add, then one fp32 multiply, no FMA --, then with relu != 0 the positive part
 * (-0 and NaN become +0).  backward: g[i] = scale * dy[i], and with relu != 0 g[i] = 0 where y[i] <= 0 (y: forward's result; it is
 * read only with relu).  The gradient is the same for both operands: the shortcut's share is added with w2l_axpy(dx, g, n, 1).
 * One launch over n floats, two reads and one write each; float4 where the three pointers share their phase against 16 bytes (a
 * scalar head up to the first aligned element, a scalar tail), element by element where they do not.  y may be exactly a or
 * exactly b, g may be exactly dy; any other overlap is the caller's error.  W2L_EINVAL, before any launch: a non-finite scale; a
 * null pointer with n > 0.  n == 0 launches nothing. */
int w2l_residual_join_forward(float* y, const float* a, const float* b, size_t n, float scale, int relu, w2l_stream_t stream);
int w2l_residual_join_backward(float* g, const float* dy, const float* y, size_t n, float scale, int relu, w2l_stream_t stream);
int w2l_fill(float* y, size_t n, float v, w2l_stream_t stream);
/* ema[i] = (float)decay * ema[i] + (float)(1 - decay) * p[i], fp32, ONE launch over a flat parameter arena: the averaged
 * "teacher" network of slimIPL (--slimIPL_ema, recipes/slimIPL/src/Train.cpp:1819-1832: one expression per parameter there).
 * ema and p need float alignment only and may sit differently against a 16-byte boundary.  n == 0: W2L_OK without a
 * launch.  A null pointer, or a decay that is NaN or outside [0, 1]: W2L_EINVAL before anything touches the device.  No
 * non-finite guard: the reference moves the average even when the optimizer's update was skipped. */
int w2l_ema_update(float* ema, const float* p, size_t n, double decay, w2l_stream_t stream);
int w2l_transpose(const float* in, float* out, int G, int R, int C, w2l_stream_t stream);
/* MFSC / log-mel front end (fl::lib::audio::Mfsc as configured by LogMelFeature.cpp:78-95, [UNVENDORED]): the linear
 * per-frame part (pre-emphasis, window, DFT) is one w2l_gemm_f32 on overlapping rows of the audio (lda = frame stride);
 * spectrum: spec[m][k] = |re + i im| (usePower: squared), zero-padded to ldOut columns; then the mel GEMM; then
 * out[b][f][t] = log(max(mel[b][t][f], floor)) in the network's input layout. */
int w2l_mfsc_spectrum(const float* reim /*[M][2*nbins]*/, float* spec /*[M][ldOut]*/, size_t M, int nbins,
                      int ldOut, int usePower, w2l_stream_t stream);
int w2l_mfsc_log_transpose(const float* mel /*[B][Tp][F]*/, float* out /*[B][F][T]*/, int B, int Tp, int T,
                           int F, float floorv, w2l_stream_t stream);
int w2l_glu_forward(const float* x, float* y, size_t M, int half, w2l_stream_t stream);
int w2l_glu_backward(const float* x, const float* dy, float* dx, size_t M, int half,
                     w2l_stream_t stream);

/* fl::WeightNorm on an internal [K][N] weight (per-column norm); norm[N], dot[N] scratch */
int w2l_weightnorm_forward(const float* v, const float* g, float* w, float* norm, int K, int N,
                           w2l_stream_t stream);
int w2l_weightnorm_backward(const float* v, const float* g, const float* norm, const float* dw,
                            float* dv, float* dg, float* dot, int K, int N, w2l_stream_t stream);
/* fl::SpecAugment (SAUG token): frequency / time masking with zeros, in place on x[B][T][F] */
int w2l_specaugment_inplace(float* x, int B, int T, int F, int fMaskF, int nFMask, int tMaskT,
                            float tMaskP, int nTMask, uint32_t seed, w2l_stream_t stream);

/* fl::SGDOptimizer + fl::clipGradNorm over a flat parameter arena
 * (recipes/slimIPL/src/Train.cpp:1791-1804). */
int w2l_sumsq(const float* g, size_t n, double* out, int zeroFirst, w2l_stream_t stream);
int w2l_sgd_step(float* p, const float* g, float* v, size_t n, float lr, float momentum,
                 float gradScale, float maxGradNorm, const double* sumsq, w2l_stream_t stream);
/* Non-finite guard + device-side batch size of a data-parallel step (Train.cpp:1651-1660, :1743-1747).
 * acc[5] doubles: in  acc[0] = sum g^2 of the network gradients, acc[1] = of the criterion gradients;
 *                 out acc[2] = clip norm^2 (acc[0] + clampCrit*acc[1]), NaN when ANY gradient or the batch size is
 *                     non-finite, acc[3] = 1 / *batchDev (0 if batchDev is null), acc[4] += 1 per skipped update.
 * w2l_sgd_step_guarded(guard = acc + 2) leaves p and v untouched when guard[0] is non-finite -- with or without
 * clipping -- and scales the gradient by guard[1] instead of gradScale when guard[1] > 0. */
int w2l_grad_guard(double* acc, const float* batchDev, int clampCrit, w2l_stream_t stream);
int w2l_sgd_step_guarded(float* p, const float* g, float* v, size_t n, float lr, float momentum,
                         float gradScale, float maxGradNorm, const double* guard, w2l_stream_t stream);
/* fl::AdagradOptimizer::step (--netoptim=adagrad, recipes/sota/2019/librivox/train_am_transformer_ctc.cfg:25-26; un-vendored
 * Flashlight class): var += g'^2, p -= lr g' / (sqrt(var) + eps) with g' = g * gradScale * clip; guard as w2l_sgd_step_guarded
 * (NULL: no guard, no clip, gradScale as given) */
int w2l_adagrad_step_guarded(float* p, const float* g, float* var, size_t n, float lr, float eps, float gradScale,
                             float maxGradNorm, const double* guard, w2l_stream_t stream);
/* fl::AdadeltaOptimizer::step (--netoptim=adadelta, recipes/sota/2019/librispeech/train_am_transformer_ctc.cfg:23-26; un-vendored
 * Flashlight class): accGrad = rho accGrad + (1-rho) g'^2, delta = sqrt(accDelta + eps) / sqrt(accGrad + eps) g', p -= lr delta,
 * accDelta = rho accDelta + (1-rho) delta^2 */
int w2l_adadelta_step_guarded(float* p, const float* g, float* accGrad, float* accDelta, size_t n, float lr, float rho,
                              float eps, float gradScale, float maxGradNorm, const double* guard, w2l_stream_t stream);
/* fl::AdamOptimizer::step with decoupled weight decay (--netoptim=adam, recipes/joint_training_vox_populi/cpc/Train.cpp:569-580;
 * [UNVENDORED] Flashlight class: this comment is the contract).  With t = the number of applied steps including this one:
 *   clr = lr sqrt(1 - beta2^t) / (1 - beta1^t) (fp64, rounded to fp32 once); p -= (weightDecay lr) p (first, with lr: the moments
 *   never see the decay); m = beta1 m + (1-beta1) g'; v = beta2 v + (1-beta2) g'^2; p -= clr m / (sqrt(v) + eps), eps OUTSIDE the
 *   bias correction (torch.optim.Adam divides sqrt(v) by sqrt(1 - beta2^t) first; with eps = 0 the two agree).
 * g', gradScale, maxGradNorm and guard as w2l_adagrad_step_guarded.  t = `step` (>= 1) when stepCount is NULL; else t =
 * *stepCount + 1 (device, 8 bytes), read by every thread of the one launch, and a one-thread launch behind it adds 1 to *stepCount
 * unless guard[0] is non-finite: a skipped update leaves p, m, v AND the bias correction untouched, without a host round trip.
 * One launch over n floats, 28 bytes moved per parameter; float4 where p, g, m and v share their phase against 16 bytes (a scalar
 * head up to the first aligned element), element by element where they do not.  W2L_EINVAL, before any launch: a null p, g, m or
 * v; beta1 or beta2 outside [0, 1) or NaN; eps or weightDecay negative or NaN; step == 0 without a counter.  Zero g, m and v
 * leave p bit-identical when weightDecay == 0 (0 / (0 + eps): eps == 0 gives NaN there); a zero p stays zero under weight decay. */
int w2l_adam_step_guarded(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                          float weightDecay, float gradScale, float maxGradNorm, const double* guard, uint64_t step,
                          uint64_t* stepCount, w2l_stream_t stream);

/* ------------------------------------------------------------------------
 * 3. Trainer: arch file -> module graph -> one optimisation step.
 * Mirrors buildSequentialModule (recipes/joint_training_vox_populi/cpc/SequentialBuilder.h:23-26),
 * ASGLoss / CTCLoss construction (recipes/slimIPL/src/Train.cpp:406-410) and the hot loop
 * (Train.cpp:1454-1804).  The caller owns all device memory: query sizes, allocate, bind.
 * params / grads / momentum are flat arenas [network params | criterion params]; the
 * data-parallel all-reduce is ONE collective over `grads` between forward_backward and update.
 * ---------------------------------------------------------------------- */
const char* w2l_host_last_error(void);

/* ---- FLAC decoding (host side of the input pipeline).  Replaces: fl::pkg::speech::loadSound through libsndfile for
 * the .flac files the recipes' lists point at (data/librispeech/utils.py:36-46).  A from-specification decoder (RFC 9639): the native
 * container, every subframe type, Rice / Rice2 residuals, all stereo decorrelations, 4-32 bits; frame CRC-8 / CRC-16 and the
 * STREAMINFO MD5 of the decoded audio are verified.  `data` is the whole file in memory. */
int w2l_flac_info(const uint8_t* data, size_t bytes, int* sampleRate, int* channels, int* bitsPerSample, uint64_t* totalSamples);
/* out[sample][channel] interleaved int32, room for `capacity` inter-channel samples; *md5: 1 signature verified, -1 the file has none
 * (a mismatch returns W2L_EINVAL, as does any malformed or corrupted frame: w2l_flac_last_error() says which) */
int w2l_flac_decode(const uint8_t* data, size_t bytes, int32_t* out, uint64_t capacity, uint64_t* decoded, int* md5);
const char* w2l_flac_last_error(void);
void* w2l_trainer_create(const char* archText, int nFeat, int nLabel, const char* criterion,
                         int scaleMode, double transdiag);
void w2l_trainer_destroy(void* h);
const char* w2l_trainer_describe(void* h);
size_t w2l_trainer_param_floats(void* h);
size_t w2l_trainer_net_param_floats(void* h);
/* floats of the gradient arena to bind: parameters + a 4-float tail; tail[0] = this rank's batch size, written by
 * forward_backward, so that ONE all-reduce over [0, grad_floats) sums gradients and batch sizes
 * (recipes/slimIPL/src/Train.cpp:1743-1747 all-reduces the batch size separately) */
size_t w2l_trainer_grad_floats(void* h);
int w2l_trainer_num_params(void* h);
int w2l_trainer_param_info(void* h, int i, char* name, int nameCap, size_t* numel, size_t* offset);
int w2l_trainer_init_params(void* h, float* h_params, uint64_t seed);
int w2l_trainer_import_param(void* h, int i, const float* h_ref, float* h_params);
int w2l_trainer_export_param(void* h, int i, const float* h_arena, float* h_ref);
/* Plans one batch geometry (B utterances of T frames, targets padded to L) and reports what to bind for it.  May be called again
 * at any time, for any other shape.  A plan KEEPS parameters, gradients and optimizer arenas (and their binding), the step count,
 * Adam's step counts, the count of skipped updates and the last gradient norm, optimizer kind and hyperparameters, the
 * mixed-precision switches, dropout overrides, gradient buckets and the linseg countdown.  It DROPS the activation arena and the
 * criterion workspace (sized for the shape before), the forward pass w2l_trainer_backward would differentiate, and the input
 * sizes: until the next w2l_trainer_bind every forward / forward_backward / backward / update / evaluate returns W2L_EINVAL
 * ("trainer not planned / bound"), and sizes are given again with w2l_trainer_set_input_sizes where they are used. */
int w2l_trainer_plan(void* h, int B, int T, int L, size_t* arenaFloats, size_t* critWsBytes, int* Tout);
/* params / momentum: w2l_trainer_param_floats floats; grads: w2l_trainer_grad_floats floats (4-float tail) */
int w2l_trainer_bind(void* h, float* params, float* grads, float* momentum, float* arena, void* critWs);
/* x: [B][NFEAT][T] (the reference's (T,NFEAT,1,B) input); target [B][L] int32, -1 padded */
int w2l_trainer_forward(void* h, const float* x, int train, const float** emission, void* stream);
int w2l_trainer_forward_backward(void* h, const float* x, const int* target, float** lossDev,
                                 void* stream);
/* backward pass of the network alone from a caller-supplied gradient of the emissions [B][T'][N] (device): the fl::Module boundary
 * for a binder that keeps its own criterion.  After w2l_trainer_forward(train = 1) of the same step; leaves the network's
 * gradients in the gradient arena (unscaled).  Replaces: fl::Variable::backward through the module graph
 * (recipes/slimIPL/src/Train.cpp:1719-1721). */
int w2l_trainer_backward(void* handle, const float* dEmission, void* stream);
/* totalBatch > 0: scale the gradients by 1/totalBatch; totalBatch <= 0: by 1 / (the all-reduced batch size in the
 * gradient arena's tail).  A non-finite gradient (or batch size) skips the update on every rank -- with or without
 * clipping -- and counts it (w2l_trainer_skipped_updates). */
int w2l_trainer_update(void* h, float lr, float lrcrit, float momentum, float maxGradNorm,
                       float totalBatch, int clampCrit, void* stream);
/* updates skipped so far, over the life of the handle: the count (and the norm w2l_trainer_grad_norm reports) lives in device
 * memory the trainer owns and survives w2l_trainer_plan / w2l_trainer_bind.  0 before the first update.  Synchronises. */
int w2l_trainer_skipped_updates(void* h, uint64_t* count, void* stream);
/* optimizer of the network / criterion parameters for w2l_trainer_update: 0 = SGD with momentum (default), 1 = Adagrad
 * (eps 1e-8; the momentum arena holds the accumulated squared gradients), 2 = Adadelta (rho 0.9, eps 1e-8; accGrad in the
 * momentum arena, accDelta in a second arena of the same size: w2l_trainer_bind_state2), 3 = Adam with decoupled weight decay
 * (w2l_adam_step_guarded; m in the momentum arena, v in the second arena; hyperparameters: w2l_trainer_set_adam).
 * Train.cpp:577-582 initOptimizer(--netoptim / --critoptim) */
int w2l_trainer_set_optimizer(void* h, int netKind, int critKind);
/* Adam's hyperparameters (defaults 0.9, 0.999, 1e-8, 0: --adambeta1 --adambeta2 --optimepsilon --weightdecay of cpc/Train.cpp:569-580).
 * weightDecay acts on the network's parameters only, as initOptimizer passes it; the criterion's Adam gets 0. */
int w2l_trainer_set_adam(void* h, float beta1, float beta2, float eps, float weightDecay);
/* Adam's applied-step counts of the network and the criterion group (what the bias correction reads).  They live on the device,
 * in a buffer the trainer owns, because w2l_trainer_update decides on the device whether an update is skipped; a skipped update
 * advances neither.  The --linseg hand-over resets them with the rest of the optimizer state.  For checkpoints; both synchronise. */
int w2l_trainer_adam_steps(void* h, uint64_t* netSteps, uint64_t* critSteps, void* stream);
int w2l_trainer_set_adam_steps(void* h, uint64_t netSteps, uint64_t critSteps, void* stream);
/* input sizes of the NEXT forward calls (device, [B] floats in any unit; NULL = every utterance fills the batch): the
 * Transformer blocks mask the padded keys as the reference's forwardSequentialModuleWithPadMask does.  Call after plan: the
 * pointer holds B floats of the planned B, so w2l_trainer_plan forgets it (back to NULL) and the caller gives the new batch's. */
int w2l_trainer_set_input_sizes(void* h, const float* inputSizesDev);
int w2l_trainer_bind_state2(void* h, float* state2);
int w2l_trainer_viterbi(void* h, const float* emission, int* path, void* stream);
/* Evaluation of a held-out batch on the planned shape: eval-mode network forward (no dropout), then the criterion's loss and
 * Viterbi path in one call (CTC: w2l_ctc_score; ASG: its loss sequence and w2l_viterbi_compute).  *lossDev [B] and *pathDev
 * [B][T'] point into the evaluation buffer (w2l_trainer_bind_eval, else one the trainer owns): valid until the next
 * w2l_trainer_evaluate of this handle, untouched by training.
 * Advances no step counter or dropout seed; the activation arena is reused, so it does not survive between a
 * w2l_trainer_forward(train = 1) and its w2l_trainer_backward.  Replaces: the reference's test() (recipes/slimIPL/src/Train.cpp:874-980). */
int w2l_trainer_evaluate(void* h, const float* x, const int* target, float** lossDev, int** pathDev, void* stream);
/* the buffer w2l_trainer_evaluate works in (loss, path, score workspace) for the planned shape, and a caller-owned one to use
 * instead of the trainer's own (mem = null: back to the trainer's own) */
size_t w2l_trainer_eval_bytes(void* h);
int w2l_trainer_bind_eval(void* h, void* mem, size_t bytes);
int w2l_trainer_set_step(void* h, uint32_t step);
/* --fl_amp_use_mixed_precision restated for bf16 (BASELINE config 3): the network's fl::Linear GEMMs multiply in bf16
 * with fp32 accumulation (w2l_set_matmul_precision scoped to the network's calls); storage, master weights, convolutions,
 * LayerNorm, the criterion (recipes/joint_training_vox_populi/cpc/Train.cpp:1184) and the optimizer stay fp32 */
int w2l_trainer_set_mixed_precision(void* h, int on);
/* second level of that mode: the wide time convolutions (w2l_conv_bf16_*) on bf16 operands too.  Acts only while
 * w2l_trainer_set_mixed_precision is on.  Call before w2l_trainer_plan: a change after it drops the plan (plan and bind again). */
int w2l_trainer_set_mixed_precision_convs(void* h, int on);
/* Weight-gradient stream (on by default): the fp32 training backward enqueues the products that feed nothing before the optimizer
 * -- the weight and bias gradients of the TDS blocks' Linears and of plain Linear layers, the filter gradients of the TDS and C2
 * convolutions -- on a non-blocking side stream the network owns, and makes `stream` wait for it before
 * w2l_trainer_forward_backward / w2l_trainer_backward return: whatever the caller enqueues on `stream` afterwards sees every
 * gradient, and a gradient bucket's event (w2l_trainer_set_grad_buckets) fires once both streams have finished the bucket.  Same
 * kernels, same results, bit for bit.  Stays on `stream` alone: the mixed-precision mode, and any step while
 * w2l_profile_enable(1) is in force (the per-launch brackets time one kernel at a time).  W2L_EINVAL: null handle.
 * Host-only, takes effect at the next backward; like every call on one handle, not concurrently with a step of it. */
int w2l_trainer_set_weight_grad_stream(void* h, int on);
/* The gradient of the network's INPUT, which training has no use for: off by default, and then no layer in front of the first one
 * with parameters computes a data gradient.  On: every backward from the next one on runs them all and leaves the input's gradient
 * in the activation arena, frame-major [B][T][NFEAT] (the input itself arrives time-fastest, [B][NFEAT][T]);
 * w2l_trainer_input_gradient hands out the device pointer, valid until the next pass or plan (null before the first such
 * backward).  Parameter gradients are the same bits either way.  W2L_EINVAL: null handle / null result.  Host-only. */
int w2l_trainer_set_input_gradient(void* h, int on);
int w2l_trainer_input_gradient(void* h, const float** dInput);
/* slimIPL's dynamic dropout (--slimIPL_dyn_dropout, recipes/slimIPL/src/Train.cpp:1141-1168 with the recipe plugin's
 * 100h_supervised_slimipl.cpp:41-58): the probabilities the `TR` layers -- and only they -- use from the next forward on.  A
 * negative value restores that layer's arch value.  No new plan: a trainer with the override set computes, bit for bit, what a
 * trainer built from the arch text with these numbers in its `TR` lines computes at the same step and seed.  W2L_EINVAL: a
 * value that is NaN or >= 1. */
int w2l_trainer_set_dropout(void* h, double pDropout, double pLayerDrop);
/* gradient norm seen by the last w2l_trainer_update (before the 1/totalBatch scale; taken on every update).  A
 * non-finite norm means the update was SKIPPED on every rank (the norm is taken on the all-reduced gradient):
 * the counterpart of the reference's NaN guards, recipes/slimIPL/src/Train.cpp:1651-1660, :1686-1698. */
int w2l_trainer_grad_norm(void* h, double* norm, void* stream);
/* --linseg=n (recipes/slimIPL/src/Train.cpp:589-617, :1866-1883): the first n updates of an ASG run use
 * LinSegCriterion on the ASG criterion's own transitions.  Call before w2l_trainer_plan. */
int w2l_trainer_set_linseg(void* h, uint32_t updates);
/* Data-parallel overlap (replaces fl::CoalescingReducer, recipes/slimIPL/src/Train.cpp:195, :1721-1735):
 * bucket k = [offsets[k], offsets[k+1]) of the flat gradient arena (ascending float offsets; the last
 * bucket runs to the end).  forward_backward records one event per bucket on its stream as soon as every
 * gradient at offset >= offsets[k] is final (backward walks the layers last to first);
 * wait_bucket makes `stream` (the collective's stream) wait for bucket k.  n = 0 removes the hooks. */
int w2l_trainer_set_grad_buckets(void* h, int n, const size_t* offsets);
int w2l_trainer_wait_bucket(void* h, int k, void* stream);
/* roofline instrumentation: bracket every MFMA GEMM launch with hipEvents on its stream */
int w2l_profile_enable(int on);
int w2l_profile_report(int* launches, double* totalMs, double* totalFlops); /* kind 0 */
/* kind: 0 = 128x128 MFMA GEMM, 1 = skinny implicit GEMM, 2 = TDS slab convolution (work = FLOPs),
 * 3 = FCC transition stream (work = algorithmic bytes), -1 = all */
int w2l_profile_report_kind(int kind, int* launches, double* totalMs, double* totalWork);
/* per-launch rows of one kind (bench.py's per-shape table of the dominant kernel): ms[i], work[i], dims[4 i ..] = M, N, K, kernel tag
 * (1 = gemm128_kernel, 2 = gemm128g_kernel, 3 = gemm160_kernel 128 x 160, 4 = 160 x 128; 0 = not recorded); returns the row count */
int w2l_profile_launches(int kind, int maxRows, double* ms, double* work, int* dims);
int w2l_arch_check(const char* archText, int nFeat, int nLabel, int* numLayers);
int w2l_flags_check(const char* flagsText, int* numFlags);

/* ---- chunked streaming forward (csrc/host/stream.cpp, csrc/stream.hip) --------------------------------------------------
 * A streaming SESSION runs the network of an arch file on audio as it arrives: S slots (concurrent streams), at most maxChunk
 * input frames per slot and step.  Parameter order and layout are the trainer's, so a checkpoint's arena loads unchanged.
 * For any utterance and ANY split of it into chunks the concatenated emissions equal w2l_trainer_forward(train = 0) of that
 * utterance alone (fp32 parity, not bitwise: kernel variants depend on the row count) and the frame count equals its Tout.
 * Streamable lines: V, RO, SAUG, DO (identity in eval), PD on the time axis, C / C1 / C2 with explicit padding (or SAME at
 * stride 1), R, LN without the time axis, TDS with lnIncludeTime = 0, L, WN around C / L.  Any other line -- TR, M, GLU, LN over
 * time, TDS with lnIncludeTime = 1, SAME padding at a stride above 1 -- is refused at creation with W2L_EUNSUPPORTED and a
 * w2l_host_last_error() that names the line; so is a trainer in mixed-precision mode by w2l_stream_create_for_trainer (fp32 only;
 * the _ex calls below open mixed precision).
 * create / create_for_trainer / query / counts / slot_state / reset are host arithmetic and need no device.
 *   w2l_stream_create(archText, ...)       parameters come from w2l_stream_bind
 *   w2l_stream_create_for_trainer(h, ...)  arch of the trainer; parameters are the trainer's bound arena at every step unless
 *                                          w2l_stream_bind gives others.  The trainer must outlive the session.
 *   w2l_stream_query                       maxOut (emission frames a slot can get from one step) and the state bytes for
 *                                          (arch, slots, maxChunk) without keeping a session
 *   w2l_stream_bind                        params: device arena of w2l_stream_param_floats floats (may be NULL over a trainer);
 *                                          state: device buffer of w2l_stream_state_bytes, 256-byte aligned, the session's
 *                                          alone (carries, windows, activations); contents need no initialisation
 *   w2l_stream_step                        x: device [S][nFeat][maxChunk] float32, only the first n[s] columns of slot s are
 *                                          used; n / start / finish / nOut: HOST int [S] (start, finish may be NULL = all 0).
 *                                          start[s]: the slot begins a new utterance, its state is discarded; finish[s]: the
 *                                          frames given are the utterance's last -- the network flushes and the slot closes.
 *                                          *out: device [S][maxOut][nLabel] inside the state buffer (NULL when no slot had
 *                                          work), rows [0, nOut[s]) of slot s are that slot's new emission frames; valid until
 *                                          the next step.  nOut is host arithmetic: the step never synchronises.  Plain launches
 *                                          on `stream` (use ONE stream per session); the count table of all layers goes to the
 *                                          device with one async copy from pinned memory.
 *                                          W2L_EINVAL before anything is enqueued: n[s] outside 0..maxChunk, frames or finish
 *                                          for a slot that was never started, null pointers.
 *   w2l_stream_counts                      the bookkeeping of a step alone (advances the host state exactly as a step would)
 *   w2l_stream_slot_state                  active flag and the carry frame count of each time-extent layer of a slot
 *   w2l_stream_reset                       closes a slot and discards its state
 * w2l_stream_window: the hand-over kernel (see csrc/stream.hip): window = carry ++ new ++ zeros, the next carry and a TDS
 * block's residual frames in one launch; tab: S device entries {carry frames | zero-carry flag << 30, new, nIn, consumed}. */
int w2l_stream_create(const char* archText, int nFeat, int nLabel, int slots, int maxChunk, void** session);
int w2l_stream_create_for_trainer(void* trainer, int slots, int maxChunk, void** session);
void w2l_stream_destroy(void* session);
int w2l_stream_query(const char* archText, int nFeat, int nLabel, int slots, int maxChunk, int* maxOut, size_t* stateBytes);
int w2l_stream_max_out(void* session);
size_t w2l_stream_state_bytes(void* session);
size_t w2l_stream_param_floats(void* session);
int w2l_stream_num_time_layers(void* session);
int w2l_stream_bind(void* session, const float* params, void* state, size_t stateBytes);
int w2l_stream_counts(void* session, const int* n, const int* start, const int* finish, int* nOut);
int w2l_stream_slot_state(void* session, int slot, int* active, int* carry, int carryCap);
int w2l_stream_step(void* session, const float* x, const int* n, const int* start, const int* finish, const float** out, int* nOut,
                    void* stream);
int w2l_stream_reset(void* session, int slot);
int w2l_stream_window(const float* src, int srcRows, const float* carryIn, float* carryOut, int carryCap, float* win, int W,
                      float* res, int resShift, int To, const int* tab, int S, int F, w2l_stream_t stream);
/* Precision is a property of a session, chosen at creation through the _ex calls.  W2L_STREAM_FP32: exactly the calls above.
 * W2L_STREAM_BF16: the session computes what the mixed-precision eval forward rounds (w2l_trainer_set_mixed_precision): bf16 operands
 * for every fl::Linear product and for every convolution that has a bf16 kernel at the window's geometry (w2l_tds_conv_bf16_*);
 * fp32 accumulation, LayerNorm, residuals, carries, hand-over kernel and count arithmetic; lin1's output of a TDS block only as its
 * bf16 row image.  Its emissions equal the mixed-precision w2l_trainer_forward(train = 0) within the mixed-precision bar (2e-3 of the
 * largest magnitude), frame counts exactly -- in fact bit for bit on the recipe's shapes: the products run on w2l_gemm_bf16_smallm
 * up to 96 rows and on w2l_gemm_bf16 above (where the tile kernel is faster), and the two give the same bits.
 *   A BF16 SESSION HOLDS A SNAPSHOT OF THE MODEL.  On the first step after w2l_stream_bind, on that step's stream, it copies the
 *   parameter arena into its own state and writes the bf16 weight images from the copy; no later step reads the caller's
 *   parameters or converts a weight.  This differs from an FP32 session over a trainer, which reads the trainer's live arena at
 *   every step: a BF16 session shows further training only after w2l_stream_refresh_weights (pure host: it marks the snapshot
 *   stale, the next step takes it again; a no-op for FP32 and for an unbound session).  The state is larger by the copy
 *   (w2l_stream_state_bytes / w2l_stream_query_ex tell).
 *   Over a trainer, BF16 requires the trainer's mixed-precision mode to be ON (W2L_EINVAL otherwise, at creation and at a step:
 *   the contract stays "the session equals this trainer's own forward") and its second level (w2l_trainer_set_mixed_precision_convs)
 *   to be OFF (W2L_EUNSUPPORTED, named in the error text: the wide-convolution scratch is not planned for sessions).  FP32 over a
 *   mixed-precision trainer stays refused with W2L_EUNSUPPORTED. */
enum { W2L_STREAM_FP32 = 0, W2L_STREAM_BF16 = 1 };
int w2l_stream_create_ex(const char* archText, int nFeat, int nLabel, int slots, int maxChunk, int precision, void** session);
int w2l_stream_create_for_trainer_ex(void* trainer, int slots, int maxChunk, int precision, void** session);
int w2l_stream_query_ex(const char* archText, int nFeat, int nLabel, int slots, int maxChunk, int precision, int* maxOut,
                        size_t* stateBytes);
int w2l_stream_refresh_weights(void* session);

/* ---- one descriptor call for every whole-utterance beam search (csrc/criterion_beam_entry.hpp) ---------------------------
 * THE CONTRACT is by reference to the named entry points above and to nothing else: w2l_beam_search is the call that
 * (trans ? asg : ctc, kind, family) names, with that call's refusals in that call's order and that call's bytes in labels,
 * lengths, scores, lmScores, words and wordCounts; w2l_beam_search_workspace_size is that call's size function.
 *   family NARROW, WIDE, XL   the *_sil entry point with that family; without a score (silToken == -1 or silScore == 0) that
 *                             is the plain sibling.  family MT: the *_mt entry point.
 *   kind PLAIN   w2l_ctc_beam_search*, or w2l_asg_beam_search* with lm == NULL.   LM: w2l_ctc_beam_search_lm*, w2l_asg_beam_search*.
 *        LEX     w2l_*_beam_search_lex*.   LEXTOK: w2l_*_beam_search_lextok; with family XL or MT W2L_EUNSUPPORTED after every
 *                W2L_EINVAL, as family 2 is there, and a workspace size of 0.
 * Checked first, W2L_EINVAL: desc == NULL or family or kind out of range (a size of 0); a field the chosen search does not take
 * that is not NULL / 0, the rule of W2L_BEAM_PLAIN below -- PLAIN: lm, lmHasEos, lmWeight, classScore, eosScore (CTC: lmScores
 * too); PLAIN and LM: lexicon, wordScore, maxWords, words, wordCounts; LEX and LEXTOK: classScore.  trans == NULL: CTC. */
typedef enum { W2L_BEAM_NARROW = 0, W2L_BEAM_WIDE = 1, W2L_BEAM_XL = 2, W2L_BEAM_MT = 3 } w2l_beam_family;
typedef enum { W2L_SEARCH_PLAIN = 0, W2L_SEARCH_LM = 1, W2L_SEARCH_LEX = 2, W2L_SEARCH_LEXTOK = 3 } w2l_beam_search_kind;
typedef struct {
  int family, kind;
  int B, T, N;
  const float* input;
  const int* frames;
  const float* trans;
  int beam, beamToken;
  float threshold;
  int logAdd, normalize, nbest, maxLen;
  const void* lm;
  int lmHasEos;
  float lmWeight;
  const float* classScore;
  float eosScore;
  const void* lexicon;
  float wordScore;
  int* labels;
  int* lengths;
  float* scores;
  float* lmScores;
  int maxWords;
  int* words;
  int* wordCounts;
  int silToken;
  float silScore;
} w2l_beam_search_desc;
size_t w2l_beam_search_workspace_size(const w2l_beam_search_desc* desc);
int w2l_beam_search(const w2l_beam_search_desc* desc, void* workspace, w2l_stream_t stream);

/* ---- incremental CTC beam search for streaming (csrc/criterion_beam_stream.hpp) -----------------------------------------
 * A beam SESSION has S slots; a slot holds the search state of one utterance in progress.  A step advances every slot by the
 * emission frames it received; a result can be asked for at any time.
 * THE CONTRACT.  Take any slot and any split of its utterance's F emission frames into chunks (chunks of 0 frames count), with
 * the other slots started, idle or mid-utterance at any other phase.  The result asked for after those F frames is the
 * whole-utterance search of the same variant at B = 1, T = F, frames = NULL over the concatenated rows (in a buffer that begins
 * at a 16-byte boundary, as every allocation does: with normalize the whole searches sum a row's exponentials in an order that
 * follows from the row's address modulo 16 bytes, and the session takes the order of such a buffer), with the same beam,
 * beamToken, threshold, logAdd, normalize, nbest, maxLen and LM / lexicon arguments: labels, lengths, scores, lmScores, words
 * and wordCounts are equal BIT FOR BIT, in both logAdd modes (every value is made by the same device code in the same order;
 * node ids of the prefix table differ, and no output or decision depends on them).  A partial result is the same statement
 * with F = the frames fed so far, the end rule included: the lexicon search drops unfinished words, the EOS term is added
 * when lmHasEos.  Asking changes nothing: the same question twice gives the same bytes and later steps behave as if nobody had
 * asked.  A slot that was started and has had 0 frames returns what the end rule gives on the starting beam -- the empty prefix
 * (length 0, score 0 plus the EOS term, 0 words) in row 0, empty rows below -- the one value the whole searches cannot state,
 * since they refuse T = 0.  A slot that was never started, or was reset, returns empty rows (length -1, score -inf, labels -1).
 * Variants (all on the narrow kernels, beam and beamToken <= 64):
 *   W2L_BEAM_PLAIN  w2l_ctc_beam_search; lmScores is 0 for live rows, -inf for empty ones (as w2l_asg_beam_search without an LM).
 *                   lm, lexicon, classScore NULL, every score argument 0.
 *   W2L_BEAM_LM     w2l_ctc_beam_search_lm (lm, lmHasEos, lmWeight, classScore or NULL, eosScore).
 *   W2L_BEAM_LEX    w2l_ctc_beam_search_lex (lm, lmHasEos, lmWeight, lexicon, wordScore, eosScore).
 * lm / lexicon / classScore are device tables that must outlive the session.
 *   w2l_beam_session_state_bytes  the state buffer's size for a descriptor; 0 for one the session refuses.  Every part is
 *                                 256-byte aligned: 3 S ints; lse, lpb [S][maxChunk] and tokLp, tokC [S][maxChunk][K] (K =
 *                                 min(beamToken, N - 1)) for a step's row pass; S prefix tables of cap 8-byte edges (cap = the
 *                                 power of two >= max(64, 2 maxFrames beam)); S ints; 11 beam arrays [S][64] of 4 bytes.
 *   w2l_beam_session_bind         state: device buffer, 256-byte aligned, the session's alone; contents need no initialisation.
 *                                 Binding closes every slot.
 *   w2l_beam_session_step         emissions: device [S][maxChunk][N], rows [0, h_n[s]) of slot s are its new frames (a session
 *                                 with maxChunk = w2l_stream_max_out takes *out and nOut of w2l_stream_step as they are);
 *                                 h_n, h_start: HOST int [S] (h_start may be NULL = all 0).  h_start[s]: the slot begins a new
 *                                 utterance from the empty prefix before this step's frames.  At most two launches plus the
 *                                 clears of starting slots' tables, plain launches on `stream` (use ONE stream per session);
 *                                 the count table goes to the device with one async copy from pinned memory.  Never
 *                                 synchronises, allocates nothing.
 *   w2l_beam_session_counts       the bookkeeping of a step alone (host arithmetic, needs no device or bound state)
 *   w2l_beam_session_result       outputs for all S slots, [S][nbest]... as the whole searches lay out [B][nbest]...; one
 *                                 launch; reads state only.  words / wordCounts / maxWords: W2L_BEAM_LEX only (else ignored).
 *   w2l_beam_session_frames       frames fed to a slot since its start
 *   w2l_beam_session_reset        closes a slot
 * Refusals, all before anything is enqueued or any count moves (w2l_host_last_error() says which).  W2L_EINVAL: the whole
 * searches' argument rules; h_n[s] outside 0..maxChunk; frames for a slot that was never started; a step that would take a slot
 * past maxFrames (the message names the slot and the limit); a step or a result before bind; a state buffer that is too small
 * or misaligned; nbest outside 1..beam; labels / lengths / scores / lmScores, or the lexicon variant's words / wordCounts,
 * missing.  W2L_EUNSUPPORTED: beam or beamToken (after clipping to N - 1) above 64, an unknown variant, maxFrames * beam > 2^29.
 * A state buffer damaged between calls gives wrong hypotheses, never a spin or an access outside the buffer and the tables. */
typedef enum { W2L_BEAM_PLAIN = 0, W2L_BEAM_LM = 1, W2L_BEAM_LEX = 2 } w2l_beam_variant;
typedef struct {
  int slots, maxChunk, maxFrames, N;
  int beam, beamToken;
  float threshold;
  int logAdd, normalize, variant;
  const void* lm;
  int lmHasEos;
  float lmWeight;
  const float* classScore;
  float eosScore;
  const void* lexicon;
  float wordScore;
} w2l_beam_session_desc;
int w2l_beam_session_create(const w2l_beam_session_desc* desc, void** session);
void w2l_beam_session_destroy(void* session);
size_t w2l_beam_session_state_bytes(const w2l_beam_session_desc* desc);
int w2l_beam_session_bind(void* session, void* state, size_t bytes);
int w2l_beam_session_step(void* session, const float* emissions, const int* h_n, const int* h_start, w2l_stream_t stream);
int w2l_beam_session_counts(void* session, const int* h_n, const int* h_start);
int w2l_beam_session_result(void* session, int nbest, int maxLen, int* labels, int* lengths, float* scores, float* lmScores,
                            int maxWords, int* words, int* wordCounts, w2l_stream_t stream);
int w2l_beam_session_frames(void* session, int slot, int* h_frames);
int w2l_beam_session_reset(void* session, int slot);

/* ---- the wide beam session: the incremental form of the wide CTC searches (csrc/criterion_beam_stream.hpp) ---------
 * w2l_beam_session_create_wide makes a session with the protocol above -- bind / step / counts / result / frames / reset / destroy
 * take either kind of session and dispatch on it -- whose beam goes up to 1024 (beamToken, after clipping to N - 1, up to 64 as in
 * the wide searches).
 * THE CONTRACT is the narrow session's with one name changed: for any slot, any split of its F frames into chunks (empty chunks
 * count) and the other slots at any phase, the result is the whole-utterance search of the same variant ON THE WIDE KERNELS at
 * B = 1, T = F, frames = NULL over the concatenated rows in a buffer that begins at a 16-byte boundary -- W2L_BEAM_PLAIN:
 * w2l_ctc_beam_search_wide, W2L_BEAM_LM: w2l_ctc_beam_search_lm_wide, W2L_BEAM_LEX: w2l_ctc_beam_search_lex_wide -- and labels,
 * lengths, scores, lmScores, words and wordCounts are equal BIT FOR BIT in both logAdd modes, the end rule included.  Partial
 * results, "asking changes nothing", the empty prefix in row 0 of a started slot without frames, the empty rows of a slot that
 * was never started or was reset, nbest up to the beam, and W2L_BEAM_PLAIN's lmScores (0 for live rows, -inf for empty ones) read
 * as above.  At a beam up to 64 a wide and a narrow session return the same bytes.
 *   w2l_beam_session_wide_state_bytes  the state buffer's size; 0 for a descriptor the wide session refuses.  Every part is
 *                                 256-byte aligned: 3 S ints; lse, lpb [S][maxChunk] and tokLp, tokC [S][maxChunk][K] (K =
 *                                 min(beamToken, N - 1)); S prefix tables of cap 8-byte edges (cap = the power of two >=
 *                                 max(64, 2 maxFrames beam)); S candidate lists of beam K slots + beam 8-byte keys (slots = 7
 *                                 for W2L_BEAM_LEX, else 1: one frame's scratch, not carried); S ints; 8 beam arrays [S][beam] of
 *                                 4 bytes, 10 for W2L_BEAM_LEX.  At beam 1024 and maxFrames 4096 a slot's prefix table is 2^23
 *                                 edges = 64 MiB, its candidate list with a lexicon (K = 64) 3.6 MiB.
 * A step is the table copy, one clear per run of adjacent starting slots, the row pass and ONE scan launch (a workgroup of 1024
 * threads per slot; its 64 or 72 KiB of dynamic LDS are asked for at bind); a result is the table copy and one launch.  Never
 * synchronises, allocates nothing after bind.
 * Refusals are the narrow session's with two limits changed: W2L_EUNSUPPORTED for beam above 1024, and for beamToken (after
 * clipping to N - 1) above 64; maxFrames * beam > 2^29 stays W2L_EUNSUPPORTED.  w2l_beam_session_create keeps refusing beam > 64.
 * A state buffer damaged between calls gives wrong hypotheses, never a spin or an access outside the buffer and the tables. */
int w2l_beam_session_create_wide(const w2l_beam_session_desc* desc, void** session);
size_t w2l_beam_session_wide_state_bytes(const w2l_beam_session_desc* desc);

/* ---- the many-token beam session: the incremental form of the many-token CTC searches (csrc/criterion_beam_stream.hpp,
 * csrc/criterion_beam_xl.hpp) ----------------------------------------------------------------------------------------
 * w2l_beam_session_create_mt makes a session with the protocol above -- bind / step / counts / result / frames / reset / destroy /
 * commit_bytes / commit / committed take any kind of session and dispatch on it -- whose beam goes up to 8192 and whose beamToken
 * (after clipping to N - 1) up to 256, with the silence score of the many-token searches: the streaming recipes' 500 / 100.  The
 * descriptor keeps its layout; silToken / silScore are arguments.
 * THE CONTRACT is the wide session's with one name changed: for any slot, any split of its F frames into chunks (empty chunks
 * count) and the other slots at any phase, the result is the whole-utterance search of the same variant ON THE MANY-TOKEN ENTRY
 * POINTS at B = 1, T = F, frames = NULL over the concatenated rows in a buffer that begins at a 16-byte boundary, called with the
 * same silToken / silScore -- W2L_BEAM_PLAIN: w2l_ctc_beam_search_mt, W2L_BEAM_LM: w2l_ctc_beam_search_lm_mt, W2L_BEAM_LEX:
 * w2l_ctc_beam_search_lex_mt -- and labels, lengths, scores, lmScores, words and wordCounts are equal BIT FOR BIT in both logAdd
 * modes, the end rule and the EOS term included.  Partial results, "asking changes nothing", the empty prefix in row 0 of a started
 * slot without frames, the empty rows of a slot that was never started or was reset, nbest up to the beam, and W2L_BEAM_PLAIN's
 * lmScores (0 for live rows, -inf for empty ones) read as above.  Two consequences of the many-token searches' own contract: at
 * beamToken (clipped) <= 64 and beam <= 1024 with no silence score, a many-token session and a wide session return the same
 * bytes; and silToken = -1 or silScore == 0 executes no + 0 (the session then runs with a silence class that matches no token).
 *   w2l_beam_session_mt_state_bytes  the state buffer's size; 0 for a descriptor the many-token session refuses (it does not
 *                                 depend on the silence pair).  Every part is 256-byte aligned: 3 S control ints; the chunk's row
 *                                 pass, lse, lpb [S][maxChunk] and tokLp, tokC [S][maxChunk][K] (K = min(beamToken, N - 1), up to
 *                                 256); S prefix tables of cap 8-byte edges (cap = the power of two >= max(64, 2 maxFrames beam));
 *                                 S candidate lists of beam K slots + beam 8-byte keys (slots = 7 for W2L_BEAM_LEX, else 1); S
 *                                 gone-mask areas of slots beam ceil(K / 64) 8-byte words; S stay areas of 2 beam floats (these
 *                                 three are one frame's scratch, not carried); S pairs of ints (the current half of the slot's
 *                                 beam, its entry count); the beam halves [S][2][kF][beam] of 4 bytes, kF = 9 for W2L_BEAM_LEX,
 *                                 else 8; and the arrays the result reads: [S][beam] node, total, [S] count, [S][beam] LM state, LM
 *                                 sum, and for W2L_BEAM_LEX lexicon node.  At beam 500, K = 100, maxFrames 1024 with a lexicon a
 *                                 slot is 8 MiB of table, 2.7 MiB of candidate list and 55 KiB of masks.
 * A step is the table copy, one clear per run of adjacent starting slots, the row pass and ONE scan launch (a workgroup of 1024
 * threads per slot; its dynamic LDS, 16 bytes per entry of the beam rounded up to a power of two plus 3.2 KiB, up to 131 KiB, and
 * the result's, up to 128 KiB, are asked for at bind); a result is the table copy and one launch.  Never synchronises, allocates
 * nothing after bind.
 * Refusals are the wide session's, in its order, before anything is enqueued or any count moves, with W2L_EINVAL first of all for
 * a silScore that is not finite or a silToken outside -1 .. N - 2 (the many-token searches' rule), and W2L_EUNSUPPORTED for beam
 * above 8192, for beamToken (after clipping to N - 1) above 256, and for maxFrames * beam > 2^29.  w2l_beam_session_create and
 * w2l_beam_session_create_wide keep their own limits and messages.
 * COMMIT: w2l_beam_session_commit works on a many-token session with beam <= 1024 under the contract below (exactness,
 * stability, maximality, overflow, budget), stated against a many-token session that never commits.  Above 1024 it is refused
 * with W2L_EUNSUPPORTED before anything is enqueued (the walk is an entry per thread; the message names the limit), and
 * w2l_beam_session_commit_bytes returns 0.
 * A state buffer damaged between calls gives wrong hypotheses, never a spin or an access outside the buffer and the tables. */
int w2l_beam_session_create_mt(const w2l_beam_session_desc* desc, int silToken, float silScore, void** session);
size_t w2l_beam_session_mt_state_bytes(const w2l_beam_session_desc* desc);

/* ---- committing the stable prefix of a beam session and compacting its table (csrc/criterion_beam_commit.hpp) -------
 * For either kind of session.  Every hypothesis a slot will ever return descends from one of its stored beam entries, so the
 * labels above the deepest common ancestor C of ALL stored entries (the lexicon variant's entries with an unfinished word, which
 * a result hides, included) can never change again, whatever audio follows.  w2l_beam_session_commit hands them out -- all labels
 * above C: C's own label stays back, so that no entry is left at the root with a real last label -- and rebuilds the slot's prefix
 * table with only the nodes that stored entries still descend from.  The slot's results from then on are TAILS: the labels (and
 * words) after the committed ones.  If C is the root or a child of the root, or the beam is dead, nothing is committed and the
 * table is still compacted.
 * THE CONTRACT.
 *   Exactness.   Sessions A and B have the same descriptor (but for maxFrames) and are fed the same frames; A never commits
 *                (and has the maxFrames for that), B commits at any points.  After any number of frames, for every row m of a
 *                result: B's committed labels since the slot's start followed by B's row m are A's row m; B's lengths and
 *                wordCounts plus its committed totals are A's; B's committed words followed by its row's words are A's; scores
 *                and lmScores are equal BIT FOR BIT, in both logAdd modes, all three variants, narrow and wide.  Empty rows stay
 *                empty rows (length -1: nothing is added to them).
 *   Stability.   The committed labels are a prefix of every row that A returns at any later time.
 *   Maximality.  W2L_BEAM_PLAIN and W2L_BEAM_LM: the total committed after a commit is max(0, LCP - 1), LCP the longest common
 *                prefix of ALL live rows of A's result at nbest = beam at that moment.  W2L_BEAM_LEX: at most that (hidden
 *                unfinished entries hold the cut back; homophones are different nodes with equal labels).
 *   Overflow.    A slot whose commit has more than maxLen labels or more than maxWords words is refused with W2L_EINVAL before
 *                anything of it is changed (the kernel counts first): committed wholly or not at all.  The message names the first
 *                such slot and what it needs; h_nLabels / h_nWords of a refused slot hold the NEED, h_live its unchanged live
 *                count, and its totals do not move.  The other flagged slots of the call are committed as usual.
 *   Budget.      The table after a commit holds `live` nodes.  The slot may then take maxFrames - ceil(live / beam) further frames
 *                before its next commit (the table then holds at most live + beam * frames <= beam * maxFrames <= cap / 2 nodes);
 *                a step past that is refused with W2L_EINVAL, naming the slot, and w2l_beam_session_counts follows the same rule.
 *                A slot that has not committed since its start keeps the maxFrames rule and its message.  Start, reset and bind
 *                zero the committed totals and the budget.  w2l_beam_session_frames keeps returning the frames since the start.
 *   w2l_beam_session_commit_bytes  the scratch for ONE slot, every part 256-byte aligned: 4 S ints; a table of cap 8-byte edges;
 *                                 a label stack [maxFrames][64] ints (wide: [maxFrames][beam]).  At beam 1024 and maxFrames
 *                                 4096: 64 MiB + 16 MiB.  A caller buffer of its own, so the state sizes do not move.
 *   w2l_beam_session_commit       h_commit: HOST int [S], non-zero = commit this slot; NULL = every started slot.  A flagged slot
 *                                 that was never started, or was reset, does nothing and reports 0 / 0 / 0.  labels: device
 *                                 [S][maxLen], words: device [S][maxWords] (W2L_BEAM_LEX only, else ignored): row s holds what
 *                                 THIS call committed for slot s, in order, padded with -1 (rows of slots that did nothing are
 *                                 not written).  h_nLabels, h_nWords (may be NULL), h_live (may be NULL): HOST int [S].  Flagged
 *                                 slots are processed one after another on `stream` against the one scratch: a clear, one
 *                                 workgroup that finds the cut, writes the labels and rebuilds the table, one copy pass.  THIS IS
 *                                 THE ONE SESSION CALL THAT SYNCHRONISES: it waits for `stream` once, at its end, to bring the
 *                                 counts and live to the host.  A session that never calls it runs exactly the launches it ran
 *                                 before.
 *   w2l_beam_session_committed    labels and words (either may be NULL) committed by a slot since its start
 * Refusals (W2L_EINVAL, before anything is enqueued): a call before bind; scratch missing, misaligned or smaller than
 * w2l_beam_session_commit_bytes; maxLen < 1; labels missing; words missing or maxWords < 1 for W2L_BEAM_LEX; h_nLabels missing.
 * A state buffer damaged between calls gives wrong labels, never a spin or an access outside the buffers: every walk up a table
 * stays inside it and ends after as many labels as the slot has had frames. */
size_t w2l_beam_session_commit_bytes(void* session);
int w2l_beam_session_commit(void* session, const int* h_commit, void* scratch, size_t scratchBytes, int maxLen, int* labels,
                            int maxWords, int* words, int* h_nLabels, int* h_nWords, int* h_live, w2l_stream_t stream);
int w2l_beam_session_committed(void* session, int slot, int* h_labels, int* h_words);

/* ---- streaming log-mel front end (csrc/host/feat_stream.cpp, csrc/feat_stream.hip) ----------------------------
 * A feature session turns audio chunks of `slots` concurrent streams into MFSC frames on the device, one launch per step: the
 * first module of the reference's streaming pipeline (LogMelFeature: buffer the samples, produce numFrames(buffered) frames,
 * consume numFrames x stride samples, keep the rest).  For any utterance and any split of it into chunks the concatenated frames
 * are the same, bit for bit, and equal the whole-utterance Mfsc up to summation order.  No normalisation: as before, that is the
 * caller's.  The protocol is w2l_stream_*'s:
 *   w2l_feat_desc                   what Mfsc derives: frameSize N and frameStride St in samples, nbins, ldSpec (rows of H), numFilters
 *                                   F, usePower, melFloor.  Accepted: 1 <= St <= N <= 512, nbins <= 257, nbins <= ldSpec, F <= 128,
 *                                   melFloor > 0.  Larger: W2L_EUNSUPPORTED, w2l_host_last_error() names the field; sizes below 1,
 *                                   St > N, nbins > ldSpec, melFloor <= 0: W2L_EINVAL.
 *   w2l_feat_session_query          maxOut = (maxSamples - 1) / St + 1 (the frames N - 1 carried and maxSamples new samples can
 *                                   hold) and the state bytes.  Host arithmetic, like create, counts, slot_state and reset.
 *   w2l_feat_session_bind           G: device [N][2 nbins] (real | imaginary columns), H: device [ldSpec][F], exactly as Mfsc holds
 *                                   them (the session's "weights": it keeps the pointers); state: device buffer of
 *                                   w2l_feat_session_state_bytes, 256-byte aligned, no initialisation needed.  Bind zeroes the
 *                                   output area (and waits for that).
 *   w2l_feat_session_step           pcm: device [S][maxSamples], W2L_PCM_F32 float32 or W2L_PCM_S16 int16 (scaled by exactly
 *                                   1 / 32768), the first n[s] samples of slot s are used, 0 <= n[s] <= maxSamples.  n, start,
 *                                   finish (either flag array may be NULL) and nOut are HOST int [S].  Per slot: start empties the
 *                                   carry; have = carry + n; nOut = have < N ? 0 : 1 + (have - N) / St; the slot consumes nOut St
 *                                   samples and carries the rest (< N); finish drops the rest after the step's frames and closes
 *                                   the slot, as the whole-utterance Mfsc drops the same tail.  *out: device [S][F][maxOut] inside
 *                                   the state -- the layout w2l_stream_step takes as x, so a session with maxChunk == maxOut
 *                                   consumes (*out, nOut) as they are.  Columns at or beyond nOut[s] are not written.  One launch
 *                                   and one async copy of the count table (pinned ring); never synchronises.
 *   w2l_feat_session_counts         the bookkeeping of a step alone (advances the host state exactly as a step would)
 *   w2l_feat_session_slot_state     active flag and carried sample count of a slot
 *   w2l_feat_session_reset          closes a slot and discards its carry
 * Refused with W2L_EINVAL before anything is enqueued or any count moves: null pointers, n[s] outside 0..maxSamples, a slot fed
 * or finished before it was started, a step before bind.
 * w2l_feat_stream_frames is the kernel behind a step (tab: device int [S][4] = carried samples, new samples, frames, flags with
 * bit 0 = the current carry buffer and bit 1 = the slot has work; the next carry goes to the other buffer);
 * w2l_feat_stream_tile_rows the frames one workgroup computes. */
enum { W2L_PCM_F32 = 0, W2L_PCM_S16 = 1 };
typedef struct w2l_feat_desc {
  int frameSize, frameStride, nbins, ldSpec, numFilters, usePower;
  float melFloor;
} w2l_feat_desc;
int w2l_feat_session_query(const w2l_feat_desc* desc, int slots, int maxSamples, int* maxOut, size_t* stateBytes);
int w2l_feat_session_create(const w2l_feat_desc* desc, int slots, int maxSamples, void** session);
void w2l_feat_session_destroy(void* session);
int w2l_feat_session_max_out(void* session);
size_t w2l_feat_session_state_bytes(void* session);
int w2l_feat_session_bind(void* session, const float* G, const float* H, void* state, size_t stateBytes);
int w2l_feat_session_counts(void* session, const int* n, const int* start, const int* finish, int* nOut);
int w2l_feat_session_step(void* session, const void* pcm, int pcmType, const int* n, const int* start, const int* finish,
                          const float** out, int* nOut, w2l_stream_t stream);
int w2l_feat_session_slot_state(void* session, int slot, int* active, int* carrySamples);
int w2l_feat_session_reset(void* session, int slot);
int w2l_feat_stream_tile_rows(void);
int w2l_feat_stream_frames(const w2l_feat_desc* desc, const float* G, const float* H, const void* pcm, int pcmType, int maxSamples,
                           const int* tab, float* carry0, float* carry1, int carryLd, float* out, int maxOut, int slots,
                           w2l_stream_t stream);

/* ---- LocalNorm: windowed feature normalisation, batch and streaming (csrc/local_norm.hip, csrc/host/norm_stream.cpp)
 * The module between the log-mel features and the network in the reference's streaming pipeline (streaming::LocalNorm(nFeat, left,
 * right), inference/module/nn/LocalNorm.cpp) and the input transform of its trainer under --localnrmlleftctx / --localnrmlrightctx.
 * Features are fp32 [B][F][ld] with time fastest: (T, NFEAT, 1, B) column-major, w2l_feat_session_step's [S][NFEAT][maxOut].
 * THE CONTRACT.  Frame t of an utterance with n frames is normalised over the window lo = max(0, t - left) .. hi = min(n - 1,
 * t + right), with ONE scalar mean and deviation over all F features of the window's frames:
 *   1. Frame sums.   s_u = sum_f x[f][u] and q_u = sum_f x[f][u]^2, both in double, f ascending (the square of an fp32 is exact).
 *   2. Window sums.  S = sum_{u = lo..hi} s_u and Q = sum q_u, in double, u ascending, SUMMED DIRECTLY: differences of running
 *                    prefix sums are not allowed, their roundings depend on where the utterance began, and a frame's result is a
 *                    function of its window's frames alone.
 *   3. Moments.      cnt = (hi - lo + 1) F, mean = S / cnt, var = max(Q / cnt - mean mean, 0), sd = sqrt(var), all in double; if
 *                    sd <= (double)1e-5f then sd = 1 (the reference's kEpsilon rule, LocalNorm.cpp:18, 93-95).
 *   4. Output.       m = (float)mean, r = (float)(1.0 / sd), y[f][t] = (x[f][t] - m) * r: one fp32 subtract and one fp32
 *                    multiply, not contracted into an FMA.
 * With right = 0 this is the window of the reference's streaming module (left + 1 frames ending at t, LocalNorm.cpp:72-101), the
 * pinned definition; with right > 0 it is the window of its offline transform as recalled (that code is not in the tree).
 *   w2l_local_norm_workspace_size   B T (s, q) pairs of doubles: 16 B T bytes (0 for B or T below 1).  Host arithmetic.
 *   w2l_local_norm                  x: device [B][F][ldx], y: device [B][F][ldy]; frames: device int [B], clamped into 0..T, or
 *                                   NULL = T for every row.  Columns t >= frames[b] of y are not written.  y == x with ldy == ldx
 *                                   is allowed (the sums are complete before the first store).  workspace: device, 16-byte
 *                                   aligned.  Two launches whatever B, no atomics, never synchronises.
 * Refused before anything touches the device, with a message for w2l_host_last_error(): W2L_EINVAL for B, F, T < 1, left < 0,
 * right < 0, ldx < T, ldy < T, null pointers, a misaligned workspace and partial overlap of x and y; W2L_EUNSUPPORTED for
 * left + right + 1 > 65536 or F > 4096.
 * The session mirrors w2l_feat_session_*: `slots` concurrent streams, each with the (s, q) pairs of its last frames in a ring of
 * left + maxChunk pairs inside the caller's state buffer.
 *   w2l_norm_session_query / create right must be 0: W2L_EINVAL otherwise, as the reference's streaming LocalNorm refuses it
 *                                   (LocalNorm.cpp:33).  nfeat, slots (<= 65535), maxChunk < 1, left < 0: W2L_EINVAL; left + 1 >
 *                                   65536, nfeat > 4096, maxChunk > 65536: W2L_EUNSUPPORTED.  State bytes = align256(16 slots) +
 *                                   align256(16 slots (left + maxChunk)).  Host arithmetic, like slot_state and reset.
 *   w2l_norm_session_bind           state: device buffer of w2l_norm_session_state_bytes, 256-byte aligned, no initialisation
 *                                   needed.  Allocates the pinned tables; closes every slot.
 *   w2l_norm_session_step           x: device [S][F][ld], y: device [S][F][ldy]; h_n and h_start (may be NULL) are HOST int [S].
 *                                   The h_n[s] new frames of every slot (columns 0 .. h_n[s] of its rows) are normalised in ONE
 *                                   launch after one async copy of the table (pinned ring); h_start[s] != 0 begins a new utterance
 *                                   with this step's frames.  y == x with ldy == ld is allowed, so a step can run on the feature
 *                                   session's output before w2l_stream_step reads it.  Columns at or beyond h_n[s] are not
 *                                   written.  Never synchronises, allocates nothing.  A step without frames enqueues nothing.
 *   w2l_norm_session_slot_state     active flag and frames since the slot's start
 *   w2l_norm_session_reset          closes a slot
 * Refused with W2L_EINVAL before anything is enqueued or any count moves: null pointers, h_n[s] outside 0..maxChunk or above ld or
 * ldy, frames for a slot that was never started (or was reset), a step before bind, partial overlap of x and y; at bind a state
 * buffer that is missing, misaligned or smaller than w2l_norm_session_state_bytes.
 * THE CONTRACT of the session.  For any slot and any split of its frames into chunks (empty chunks count, the other slots at any
 * phase), the concatenated output equals w2l_local_norm with right = 0 on the whole utterance BIT FOR BIT. */
size_t w2l_local_norm_workspace_size(int B, int T);
int w2l_local_norm(int B, int F, int T, size_t ldx, const float* x, const int* frames, int left, int right, size_t ldy, float* y,
                   void* workspace, w2l_stream_t stream);
int w2l_norm_session_query(int nfeat, int slots, int maxChunk, int left, int right, size_t* stateBytes);
int w2l_norm_session_create(int nfeat, int slots, int maxChunk, int left, int right, void** session);
void w2l_norm_session_destroy(void* session);
size_t w2l_norm_session_state_bytes(void* session);
int w2l_norm_session_bind(void* session, void* state, size_t stateBytes);
int w2l_norm_session_step(void* session, const float* x, size_t ld, const int* h_n, const int* h_start, float* y, size_t ldy,
                          w2l_stream_t stream);
int w2l_norm_session_slot_state(void* session, int slot, int* active, long long* frames);
int w2l_norm_session_reset(void* session, int slot);

/* ---- CPC contrastive criterion (csrc/criterion_cpc.hip)
 * The criterion of the reference's self-supervised trainer (--criterion=cpc, recipes/joint_training_vox_populi/cpc/CPCCriterion.cpp:
 * 85-223): a span mask with a learned embedding over the encoder output, two projections into a common space, InfoNCE of every
 * masked frame against negatives drawn from the other masked frames of its utterance.  Activations are fp32 [B][T][C] (ArrayFire
 * dims (C, T, B)); the projection weights are [D][C] row-major (weight[d][c], ArrayFire dims (C, D)), the biases [D].
 * WHICH frames are masked and WHICH negatives are drawn is host logic (include/fl_compat/cpc.h): the device calls take
 *   mask      [B][T] bytes, nonzero = masked
 *   maskIndex [B][M] int, the masked frames of every utterance, strictly ascending per row, every value in [0, T)
 *   neg       [B][M][K] int, for masked position m (an index into the utterance's row of maskIndex) its K negatives, positions of the
 *             same row.  ANY value in [0, M) is accepted, m itself and repeats included: the window rule belongs to the sampler.
 * THE CONTRACT.
 *   Masking   y[b][t][:] = mask[b][t] ? emb[:] : x[b][t][:].  Backward: dx = mask ? 0 : dy; demb[c] = the sum of dy[b][t][c] over the
 *             masked frames, added in a fixed order (chunks of 64 frames upward, then the chunks upward).
 *   Loss      with idx = maskIndex[b]:  a = ctx[b][idx] Wc^T + bc and p = enc[b][idx] We^T + be, both [M][D]; every row of a and of p
 *             is divided by its L2 norm WITHOUT an epsilon, as the reference does: a zero row is outside the contract (it gives
 *             NaN).  s[m][0] = <p_m, a_m> / tau, s[m][1 + k] = <p_neg[b][m][k], a_m> / tau,
 *             loss[b] = (1 / M) sum_m (logsumexp_k s[m][k] - s[m][0]).
 *   Backward  given g [B]: denc [B][T][Ce] and dctx [B][T][Cc] -- every frame is written, the unmasked ones as exactly 0.0f --,
 *             dWe [D][Ce], dbe [D], dWc [D][Cc], dbc [D].
 *   Reproducibility  the same inputs give the same bits from run to run: no float atomics; where several anchors share a negative or
 *             one anchor names a negative twice the terms are added in a fixed order.
 *   w2l_cpc_workspace_size        bytes for forward and backward of one step; host arithmetic; 0 for a shape the calls refuse
 *   w2l_cpc_forward               loss: device [B].  The workspace keeps what the backward pass needs.
 *   w2l_cpc_backward              after w2l_cpc_forward with the same shape, maskIndex, neg, weights and workspace.  It leaves what
 *                                 the forward pass stored untouched: a second call gives the same bits.
 *   w2l_cpc_apply_mask            needs no workspace
 *   w2l_cpc_mask_workspace_size   bytes for w2l_cpc_apply_mask_backward: ceil(B T / 64) C floats; host arithmetic
 *   w2l_cpc_apply_mask_backward   dx may be dy
 * All device pointers; the workspaces are the caller's, 16-byte aligned; the calls never synchronise.  The products run on the
 * library's fp32 GEMM (w2l_gemm_f32, following w2l_set_matmul_precision like every other product).
 * Refused before anything touches the device, with a message for w2l_host_last_error(): W2L_EINVAL for null pointers, B, T, Ce, Cc,
 * C or D below 1, M < 1, M > T, K < 1, K > M, tau <= 0 or not finite, a misaligned workspace; W2L_EUNSUPPORTED for M + 2 (K + 1) >
 * 16000 (the coefficient row of one anchor lives in LDS) and for operands of 2^31 elements or more.  An index outside its range is
 * outside the contract, but never makes a call read or write outside its operands. */
size_t w2l_cpc_workspace_size(int B, int T, int Ce, int Cc, int D, int M, int K);
int w2l_cpc_forward(int B, int T, int Ce, int Cc, int D, int M, int K, float tau, const float* enc /*[B][T][Ce]*/,
                    const float* ctx /*[B][T][Cc]*/, const int* maskIndex /*[B][M]*/, const int* neg /*[B][M][K]*/,
                    const float* We /*[D][Ce]*/, const float* be /*[D]*/, const float* Wc /*[D][Cc]*/, const float* bc /*[D]*/,
                    float* loss /*[B]*/, void* workspace, w2l_stream_t stream);
int w2l_cpc_backward(int B, int T, int Ce, int Cc, int D, int M, int K, float tau, const int* maskIndex, const int* neg,
                     const float* We, const float* Wc, const float* g /*[B]*/, float* denc /*[B][T][Ce]*/, float* dctx /*[B][T][Cc]*/,
                     float* dWe, float* dbe, float* dWc, float* dbc, void* workspace, w2l_stream_t stream);
int w2l_cpc_apply_mask(int B, int T, int C, const float* x, const unsigned char* mask /*[B][T]*/, const float* emb /*[C]*/, float* y,
                       w2l_stream_t stream);
size_t w2l_cpc_mask_workspace_size(int B, int T, int C);
int w2l_cpc_apply_mask_backward(int B, int T, int C, const float* dy, const unsigned char* mask, float* dx, float* demb /*[C]*/,
                                void* workspace, w2l_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* W2L_HIP_H_ */
