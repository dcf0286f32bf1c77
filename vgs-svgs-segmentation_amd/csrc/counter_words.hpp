// counter_words.hpp -- the one map of vgs_ctx::counters (128 words of 64 bits, shared by every stage), of the pinned read-back scratch
// and of the context's event array.  Whoever needs a word, a byte of the scratch or an event takes it HERE.
//
// words    name                  written by                                          zeroed by / when                                   live beside
// -------  --------------------  --------------------------------------------------  -------------------------------------------------  ---------------------------------
// 0-1      CW_VOX_COUNTS         voxelize: k_tile_offsets (finite points, voxels);   overwritten whole by the one writer                nothing: the front of the step is
//                                SVGS grouping: k_sv_count_valid (word 0)                                                               over before the local cut starts
// 0        CW_LC_BANDED          k_localcut_dense, k_localcut_pg                     vgs_stage_localcut: memset of 0-127 on the main    every CW_LC_*, PL_W_*, CW_MG_*
// 1        CW_LC_OVERFLOW        k_localcut (a neighbourhood above its limit)        stream at its start -- the same for every CW_LC_*
//                                                                                    and PL_W_* word below; and by vgs_localcut_finish
//                                                                                    in front of the extra-large launch
// 2        CW_LC_DEGENERATE      k_localcut
// 3-6      CW_LC_WHY_*           k_localcut_wave (bail reasons), k_ho_lists (3)
// 7        CW_LC_SLOW            k_localcut, k_localcut_dense, k_localcut_pg
// 8-11     CW_LC_NABC            k_classify: LC_NCLASS class sizes of 32 bits (the
//                                lower half of word 11 is the last of them)
// 11 high  CW_LC_NG              hand-overs of the wide classes (list g)
// 12       CW_LC_NF2             dense / pair-list kernels: sent on, small | large
// 13       CW_MG_NDEFER          merge: k_cross, first pass (rows put off)           with the local cut's words (nobody else)           the local cut's hand-over kernels
// 14-15    CW_LC_NF              k_ho_lists / k_localcut_wave: LW_HO_BINS lengths
// 16-31    CW_LC_PROF            k_localcut_wave, -DVGS_PROF builds only
// 32-34    CW_MGPU_*             multigpu.hip (boundary records, bad roots, finite   each by its own memset in front of its kernel      a finished run only
//                                points of the region scan)
// 36       CW_FEAT_NUSED         features: k_compact_used                            overwritten whole                                  CW_ADJ_* (front fork: k_features
//                                                                                                                                       itself touches no counter word)
// 40-41    CW_ADJ_N1, CW_ADJ_N2  adjacency kernels (redo lists)                      vgs_run_adjacency, memset in front of each use     CW_FEAT_NUSED
// 40       CW_SVGS_OVF           SVGS neighbours: k_sv_neighbours                    its own memset
// 42       PL_W_WORK3            pair lists, third build                             with the local cut's words                         every CW_LC_*, PL_W_*
// 44-47    CW_LC_NCLS            k_count_classes: LC_NSLOT sizes of 32 bits          with the local cut's words
// 48-55    CW_MG_BASE            the merge stage (MG_W_*)                            vgs_stage_merge: memset of 48-55 on the main       the local cut's hand-over kernels
//                                                                                    stream at its start                                (CW_LC_*, PL_W_*)
// 56       CW_LC_NXL             k_localcut_pg<PG_D>: queue of the extra-large one   with the local cut's words
// 56       CW_VCCS_CHANGED       supervoxel stage: k_pcl_max_label                   its own memset
// 57       CW_LC_GATE            k_ho_lists: LcGate's word (low), ticket (high)      with the local cut's words                         merge's first pass reads it
// 58-61    PL_W_*                pairlist.hip: pool cursor, work / redo lengths      with the local cut's words
// 62       CW_LC_VOTED           k_ho_lists: voxels voted over
// 63       CW_PG_NCUT            k_localcut_pg: voxels cut
// 64-127   CW_LC_VOTE            k_localcut_wave<SAMPLED>: the samples' votes        with the local cut's words
//
// Words with two names, and why the two never coexist (all of these are issued on the main stream, or behind a host wait):
//   0-1  CW_VOX_COUNTS / CW_LC_BANDED, CW_LC_OVERFLOW: the voxelize stage (and the SVGS grouping) reads its counts back and waits before
//        the features stage starts; the local cut zeroes the words on the same stream afterwards.
//   40   CW_ADJ_N1 / CW_SVGS_OVF: the SVGS neighbour search REPLACES the adjacency kernels for method 3; each memsets the word first.
//   56   CW_LC_NXL / CW_VCCS_CHANGED: the supervoxel stage ends with a blocking read-back of the word, before the local cut of the same run
//        zeroes it; the next run's supervoxel stage starts only after the merge stage has collected the local cut (vgs_localcut_finish).
#ifndef VGS_COUNTER_WORDS_HPP_
#define VGS_COUNTER_WORDS_HPP_

enum CounterWord {
  CW_VOX_COUNTS = 0,        // 0-1
  CW_LC_BANDED = 0,
  CW_LC_OVERFLOW = 1,
  CW_LC_DEGENERATE = 2,
  CW_LC_WHY_SHRINK = 3,     // 3-6: why the lazy schedule gave a voxel up (k_ho_lists adds every hand-over it lists to the first)
  CW_LC_WHY_FULL = 4,
  CW_LC_WHY_COLLAPSE = 5,
  CW_LC_WHY_PHASEB = 6,
  CW_LC_SLOW = 7,
  CW_LC_FLAGS_END = 8,      // the finish re-reads [0, 8) behind every kernel it launches
  CW_LC_NABC = 8,           // 8-11 (low half of 11)
  CW_LC_NG = 11,            // upper half
  CW_LC_NF2 = 12,
  CW_MG_NDEFER = 13,
  CW_LC_NF = 14,            // 14-15
  CW_LC_PROF = 16,          // 16-31
  CW_LC_PROF_END = 32,
  CW_MGPU_NREC = 32,
  CW_MGPU_BAD = 33,
  CW_MGPU_NFINITE = 34,
  CW_FEAT_NUSED = 36,
  CW_ADJ_N1 = 40,
  CW_ADJ_N2 = 41,
  CW_SVGS_OVF = 40,
  PL_W_WORK3 = 42,          // the third build's work / redo list lengths (three builds of one run may overlap on their streams: the wide
                            // classes' rows, the many hand-overs' rows, the rows of the neighbourhoods the dense kernel passes on)
  CW_LC_NCLS = 44,          // 44-47 (low half of 47)
  CW_LC_NCLS_END = 48,
  CW_MG_BASE = 48,          // 48-55
  CW_MG_END = 56,
  CW_LC_NXL = 56,
  CW_VCCS_CHANGED = 56,
  CW_LC_GATE = 57,
  PL_W_CURSOR = 58,         // entries handed out
  PL_W_WORK = 59,           // length of the work list (low half), of the redo list (high half)
  PL_W_FULL = 60,           // rows that found the pool exhausted
  PL_W_WORK2 = 61,          // the second build's work / redo list lengths
  CW_LC_VOTED = 62,
  CW_PG_NCUT = 63,
  CW_LC_SNAPSHOT = 64,      // vgs_localcut_finish reads [0, 64) back in one copy
  CW_LC_VOTE = 64,          // 64-127
  CW_COUNT = 128
};
// the merge stage's words, relative to CW_MG_BASE
enum MergeWord { MG_W_NCAND = 0, MG_W_CHANGED = 1, MG_W_NROOTS = 2, MG_W_NKEPT = 3, MG_W_CHG4 = 4 /* 4-5: four 32-bit counters */, MG_W_COUNT = 8 };

// ranges that are live together must not overlap: the local cut's, the pair lists', the merge stage's and word 13, the votes
static_assert(CW_LC_SLOW < CW_LC_NABC && CW_LC_NABC < CW_LC_NG && CW_LC_NG < CW_LC_NF2 && CW_LC_NF2 < CW_MG_NDEFER && CW_MG_NDEFER < CW_LC_NF &&
              CW_LC_NF + 2 <= CW_LC_PROF, "local cut: flags, class sizes, list lengths and the merge stage's deferred count");
static_assert(CW_LC_PROF_END <= PL_W_WORK3 && PL_W_WORK3 < CW_LC_NCLS && CW_LC_NCLS_END <= CW_MG_BASE && CW_MG_BASE + MG_W_COUNT == CW_MG_END &&
              CW_MG_END <= CW_LC_NXL && CW_LC_NXL < CW_LC_GATE && CW_LC_GATE < PL_W_CURSOR, "local cut, pair lists and merge stage run side by side");
static_assert(PL_W_CURSOR < PL_W_WORK && PL_W_WORK < PL_W_FULL && PL_W_FULL < PL_W_WORK2 && PL_W_WORK2 < CW_LC_VOTED &&
              CW_LC_VOTED < CW_PG_NCUT && CW_PG_NCUT < CW_LC_VOTE && CW_LC_VOTE + 64 == CW_COUNT, "pair lists' pool words, the counts behind them, the votes");
static_assert(CW_FEAT_NUSED < CW_ADJ_N1 && CW_ADJ_N1 < CW_ADJ_N2, "front fork: the features stage's count beside the adjacency kernels' lists");
static_assert(CW_MGPU_NREC < CW_MGPU_BAD && CW_MGPU_BAD < CW_MGPU_NFINITE && CW_MGPU_NFINITE < CW_FEAT_NUSED, "multi-GPU words");

// The pinned scratch (vgs_ctx::pin): small read-backs land here.  Two halves, so that a split read-back that has not been collected yet
// survives a plain one in between.
enum {
  VGS_PIN_BYTES = 4096,
  VGS_PIN_SPLIT = 2048   // [0, SPLIT): vgs_readback, vgs_readback_on, vgs_localcut_finish_queue; [SPLIT, BYTES): vgs_readback_begin / _end
};
static_assert(CW_LC_SNAPSHOT * 8 <= VGS_PIN_SPLIT, "the local cut's snapshot fits the lower half");

// The context's events (vgs_ctx::ev), all created with timing enabled: what each marks, the stream that records it, who waits.
enum VgsEvent {
  EV_LC_BEGIN,       // local cut: in front of the stage's kernels; main stream; read by the finish's clock (VGS_T_LOCALCUT_KERNEL)
  EV_LC_FORK,        // local cut: classes formed, parameters on the device; main stream; stream2, stream3 and stream4 wait
  EV_LC_STAGGER,     // local cut: recorded on stream3 right behind its wait for the fork; the main stream waits, so that the bulk class starts a few microseconds after the others
  EV_LC_SIDE4,       // local cut, two meanings by path: pair-list path -- class C0's pair-list kernel done; shell path -- classes C0 and D done; stream4; stream2 (the wide hand-overs) and the main stream wait
  EV_LC_WIDE_CUT,    // local cut: the wide classes on stream2 are done, their hand-overs follow; stream2; the main stream waits at the join
  EV_LC_WIDE_DONE,   // local cut: everything of stream2 is queued, the wide hand-overs included; stream2; the finish waits (the main stream under VGS_NO_OVERLAP)
  EV_LC_SAMPLES_B,   // local cut: samples and class B done; stream3; the main stream waits at the join
  EV_LC_BULK_BEGIN,  // local cut: in front of the bulk class; main stream; clock only (VGS_T_LOCALCUT_BULK)
  EV_LC_BULK_END,    // local cut: behind the bulk class; main stream; stream3 waits (k_ho_lists reads every mark), and the clock
  EV_LC_HO_DONE,     // local cut: both hand-over chains of the one-wavefront classes done; stream3; the finish waits (the main stream under VGS_NO_OVERLAP)
  EV_LC_MAIN_END,    // local cut: end of the stage's main-stream work; main stream; the finish measures the tail behind it
  EV_LC_END,         // local cut: behind the finish's waits, and again behind every kernel it launches; the finish's stream; clocks only
  EV_LABELS_BEGIN,   // merge: in front of the label tail; main stream; clock only (VGS_T_LABELS)
  EV_LABELS_END,     // merge / multi-GPU relabel: behind the last kernel that wrote pt_label; main stream; label downloads on s_d2h wait, and the clock
  EV_COUNT
};

#endif
