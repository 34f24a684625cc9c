/* Re-identification: a lost track keeps its id.  A stage behind a tracker (yf_images_reid_device) that rewrites the ids of the tracker's
 * output: a newly born track whose face looks like that of a recently lost one reports the lost one's id.  Shared by the device kernel
 * (yf_images_reid.hip.h), the host entry in yf_images.hip, a host build (yf_images_host.c, which tests/test_reid_host.py checks against
 * ptq.reid_step) and a sanitizer program (tests/csrc/reid_sanitize_main.c).  Plain C, integers throughout: the kernel, the host build
 * and Python agree bit for bit.
 *
 * The reference has no tracker and no such stage: the definition is the library's own.  The three trackers (yf_images_track.h,
 * yf_images_motion.h, yf_images_assign.h) associate by box overlap alone; a face hidden for longer than max_misses steps returns under a
 * new id, and yf_images_score.h counts an identity switch.  This stage is the second look at the picture.  It works behind all three.
 *
 * INPUT.  A tracker's output as it lies -- info[f][0 .. out_cap) and out_counts[f] -- and desc[f][0 .. out_cap), the descriptors of
 * the reported boxes (yf_images_describe.h with cap = out_cap, or any 64 bytes per record with bit 0 of flags for "valid").
 *
 * STATE.  yf_reid_state per stream (5128 bytes, 8-byte aligned): clock, reserved, and YF_REID_ENTRIES = 64 entries of 80 bytes: id,
 * the identity reported (0: the entry is free); alias, the tracker id currently mapped to it; seen, the clock value when it was last
 * bound; flags, bit 0 (YFI_REID_HAS_DESC) "has a descriptor"; v[64].  All zero is the empty state.  The bytes are untrusted: whatever
 * they hold, a step reads and writes only inside them -- NO VALUE READ FROM THE STATE INDEXES ANYTHING.
 *
 * PARAMETERS.  yf_reid_params {max_distance >= 0, max_age >= 0, blend in [0, 256]}.
 *
 * DISTANCE (yfi_reid_distance).  For two descriptors a and b with A the sum of the a_i and B the sum of the b_i:
 *   d = sum over i of |(64 a_i - A) - (64 b_i - B)|,
 * the mean-removed sum of absolute differences, times 64.  Exact in int32 and at most 64 * 64 * 255.  Adding one constant to every byte
 * of a changes no term; what a brightness change does to a descriptor computed from pixels is bounded by the rounding of its bytes.
 *
 * ONE STEP of a stream.  Of frame f the first m = min(max(count, 0), out_cap, 64) records count (yfi_track_clamp); a larger count sets
 * status bit 0 (YFI_REID_ST_CLIPPED).  Each has tid = info.id and misses = info.misses.  A record with tid == 0 is VOID: its id stays 0
 * and status bit 1 (YFI_REID_ST_VOID) is set.
 *  1. clock += 1 modulo 2^32; the result is `now`.  Ages are now - seen in uint32 arithmetic.
 *  2. Bind, for the records in ascending order: a record is BOUND to the lowest entry with id != 0 and alias == tid.  Its output id is
 *     that entry's id, and seen = now.  If misses == 0 and its descriptor is valid the entry's descriptor is updated (yfi_reid_blend):
 *     per byte (old * (256 - blend) + new * blend + 128) >> 8; an entry that had no descriptor takes the new bytes as they are and
 *     gets the flag.
 *  3. Expire: every entry with id != 0 that no record bound and whose age exceeds max_age is freed: all of its 80 bytes become zero.
 *  4. Re-identify.  Candidate records: the unbound, non-void ones with misses == 0 and a valid descriptor.  Candidate entries: the
 *     unbound ones with id != 0 and a descriptor.  A pair is eligible if d <= max_distance.  Repeatedly the eligible pair of the smallest
 *     d is taken; ties go to the lowest record, then the lowest entry.  The entry gets alias = tid and seen = now, its descriptor is
 *     blended as in step 2, the record's id is the entry's id, and both leave the candidates.  (Only the taken entry's descriptor
 *     changes, so the distances may be computed once.)
 *  5. Births: the remaining unbound, non-void records in ascending order each take the lowest free entry (id == 0); if none is free,
 *     the unbound entry of the largest age, ties to the lowest index -- it always exists, because at most 64 records count and each
 *     binds at most one entry.  The new entry has id = alias = tid, seen = now, and the record's descriptor if it is valid; otherwise no
 *     descriptor (flags 0, v zero).
 * OUTPUT.  info_out[f][r] for r < m: the id replaced, hits, misses and age copied; info_out may be info itself.  what[f][r] (if given):
 * 0 void, 1 known (YF_REID_KNOWN), 2 re-identified, 3 born.  The records from m up to min(count, out_cap) -- there are some only with
 * out_cap > 64, and no tracker emits them -- are copied as they are, what 0.  The places at and beyond min(count, out_cap) are not
 * written.  status[f] (if given): 0 or the bits above.  THE RECORDS KEEP THE TRACKER'S ORDER, SO THE IDS OF A FRAME ARE NO LONGER
 * ASCENDING.
 *
 * A CALL: n = streams * steps frames in the tracker's layouts (yf_images_track.h); the steps of stream s are taken in order on
 * state[s], which is read before the first and written after the last.
 *
 * OUT OF SCOPE.  An id the tracker itself exchanged between two faces cannot be corrected: the stage sees tracker ids, and a tracker id
 * that is the alias of an entry is believed.  An entry whose track the tracker still holds over (reported with misses > 0) is bound and
 * cannot be claimed by another track.  Colour descriptors and learned embeddings are not included.  The suggested max_distance is a
 * choice made on synthetic textures (profiles/reid_bench.txt), not a figure from labelled video. */
#ifndef YF_IMAGES_REID_H
#define YF_IMAGES_REID_H
#include <string.h>
#include "yf_images_track.h"
#include "yf_images_describe.h"

#define YFI_REID_HAS_DESC 1u
#define YFI_REID_ST_CLIPPED 1           /* status bit 0: count above min(out_cap, 64) */
#define YFI_REID_ST_VOID 2              /* status bit 1: a record of tracker id 0 */
#define YFI_REID_ENTRY_WORDS 20         /* sizeof(yf_reid_entry) / 4 */
#define YFI_REID_STATE_WORDS 1282       /* sizeof(yf_reid_state) / 4 */
#define YFI_REID_MAX_DISTANCE (64 * 64 * 255)

#ifdef __cplusplus
static_assert(sizeof(yf_reid_entry) == 80 && sizeof(yf_reid_entry) == 4 * YFI_REID_ENTRY_WORDS && sizeof(yf_reid_state) == 5128 &&
              sizeof(yf_reid_state) == 4 * YFI_REID_STATE_WORDS && sizeof(yf_reid_params) == 12 && YF_REID_ENTRIES == YF_TRACK_SLOTS &&
              YF_REID_ENTRIES == YF_TRACK_MAX_DETS, "the layout include/yf_images.h states");
#else
_Static_assert(sizeof(yf_reid_entry) == 80 && sizeof(yf_reid_entry) == 4 * YFI_REID_ENTRY_WORDS && sizeof(yf_reid_state) == 5128 &&
               sizeof(yf_reid_state) == 4 * YFI_REID_STATE_WORDS && sizeof(yf_reid_params) == 12 && YF_REID_ENTRIES == YF_TRACK_SLOTS &&
               YF_REID_ENTRIES == YF_TRACK_MAX_DETS, "the layout include/yf_images.h states");
#endif

/* THE blend of one byte; blend in [0, 256]: at most (255 * 256 + 128) >> 8 = 255 */
YFI_HD uint32_t yfi_reid_blend(uint32_t old_byte, uint32_t new_byte, int blend) {
  return (old_byte * (uint32_t)(256 - blend) + new_byte * (uint32_t)blend + 128u) >> 8;
}

/* one term of THE distance: bytes a and b of descriptors with sums A and B */
YFI_HD int32_t yfi_reid_term(int32_t a, int32_t A, int32_t b, int32_t B) {
  const int32_t t = (64 * a - A) - (64 * b - B);
  return t < 0 ? -t : t;
}

/* THE distance of two descriptors of 64 bytes */
YFI_HD int32_t yfi_reid_distance(const uint8_t* a, const uint8_t* b) {
  int32_t A = 0, B = 0, d = 0;
  for (int i = 0; i < YF_DESC_BYTES; ++i) { A += a[i]; B += b[i]; }
  for (int i = 0; i < YF_DESC_BYTES; ++i) d += yfi_reid_term(a[i], A, b[i], B);
  return d;
}

/* the entry's descriptor after it has met the record's valid descriptor nv */
static inline void yfi_reid_update(yf_reid_entry* e, const uint8_t* nv, int blend) {
  if ((e->flags & YFI_REID_HAS_DESC) != 0) {
    for (int i = 0; i < YF_DESC_BYTES; ++i) e->v[i] = (uint8_t)yfi_reid_blend(e->v[i], nv[i], blend);
  } else {
    memcpy(e->v, nv, YF_DESC_BYTES);
    e->flags |= YFI_REID_HAS_DESC;
  }
}

/* THE step, sequentially: steps 1-5 above on one stream's state.  info, desc, info_out, what are the frame's rows */
static inline void yfi_reid_step(yf_reid_state* st, const yf_track_info* info, const yf_face_desc* desc, int32_t count, int out_cap,
                                 const yf_reid_params* p, yf_track_info* info_out, int32_t* what, int32_t* status) {
  const int m = yfi_track_clamp(count, out_cap);
  int bits = yfi_track_clipped(count, out_cap) ? YFI_REID_ST_CLIPPED : 0;
  yf_track_info in[YF_REID_ENTRIES];
  uint32_t out_id[YF_REID_ENTRIES];
  int kind[YF_REID_ENTRIES], valid[YF_REID_ENTRIES], bound[YF_REID_ENTRIES];
  for (int r = 0; r < m; ++r) {
    in[r] = info[r];                                                   /* info_out may be info */
    out_id[r] = 0; kind[r] = 0;
    valid[r] = (desc[r].flags & YF_DESC_VALID) != 0;
    if (in[r].id == 0) bits |= YFI_REID_ST_VOID;
  }
  for (int e = 0; e < YF_REID_ENTRIES; ++e) bound[e] = 0;
  const uint32_t now = ++st->clock;
  /* 2. bind */
  for (int r = 0; r < m; ++r) {
    if (in[r].id == 0) continue;
    int e = 0;
    while (e < YF_REID_ENTRIES && !(st->entry[e].id != 0 && st->entry[e].alias == in[r].id)) ++e;
    if (e == YF_REID_ENTRIES) continue;
    bound[e] = 1; kind[r] = YF_REID_KNOWN; out_id[r] = st->entry[e].id;
    st->entry[e].seen = now;
    if (in[r].misses == 0 && valid[r]) yfi_reid_update(&st->entry[e], desc[r].v, p->blend);
  }
  /* 3. expire */
  for (int e = 0; e < YF_REID_ENTRIES; ++e)
    if (st->entry[e].id != 0 && !bound[e] && (uint32_t)(now - st->entry[e].seen) > (uint32_t)p->max_age) memset(&st->entry[e], 0, sizeof st->entry[e]);
  /* 4. re-identify */
  int rcand[YF_REID_ENTRIES], ecand[YF_REID_ENTRIES], any = 0;
  for (int r = 0; r < m; ++r) {
    rcand[r] = kind[r] == 0 && in[r].id != 0 && in[r].misses == 0 && valid[r];
    any |= rcand[r];
  }
  if (any) {
    for (int e = 0; e < YF_REID_ENTRIES; ++e) ecand[e] = !bound[e] && st->entry[e].id != 0 && (st->entry[e].flags & YFI_REID_HAS_DESC) != 0;
    for (;;) {
      int32_t best = p->max_distance;
      int br = -1, be = -1;
      for (int r = 0; r < m; ++r) {
        if (!rcand[r]) continue;
        for (int e = 0; e < YF_REID_ENTRIES; ++e) {
          if (!ecand[e]) continue;
          const int32_t d = yfi_reid_distance(desc[r].v, st->entry[e].v);
          if (br < 0 ? d <= best : d < best) { best = d; br = r; be = e; }      /* ascending r, then e, and a strict comparison: the ties */
        }
      }
      if (br < 0) break;
      yf_reid_entry* en = &st->entry[be];
      en->alias = in[br].id; en->seen = now;
      yfi_reid_update(en, desc[br].v, p->blend);
      bound[be] = 1; ecand[be] = 0; rcand[br] = 0;
      kind[br] = YF_REID_REIDENTIFIED; out_id[br] = en->id;
    }
  }
  /* 5. births */
  for (int r = 0; r < m; ++r) {
    if (kind[r] != 0 || in[r].id == 0) continue;
    int e = 0;
    while (e < YF_REID_ENTRIES && st->entry[e].id != 0) ++e;
    if (e == YF_REID_ENTRIES) {
      uint32_t oldest = 0;
      e = -1;
      for (int k = 0; k < YF_REID_ENTRIES; ++k) {
        const uint32_t age = (uint32_t)(now - st->entry[k].seen);
        if (!bound[k] && (e < 0 || age > oldest)) { oldest = age; e = k; }
      }
      if (e < 0) continue;                                             /* not reached: fewer than 64 entries are bound here */
    }
    yf_reid_entry* en = &st->entry[e];
    memset(en, 0, sizeof *en);
    en->id = in[r].id; en->alias = in[r].id; en->seen = now;
    if (valid[r]) { en->flags = YFI_REID_HAS_DESC; memcpy(en->v, desc[r].v, YF_DESC_BYTES); }
    bound[e] = 1; kind[r] = YF_REID_BORN; out_id[r] = in[r].id;
  }
  for (int r = 0; r < m; ++r) {
    info_out[r].id = out_id[r]; info_out[r].hits = in[r].hits; info_out[r].misses = in[r].misses; info_out[r].age = in[r].age;
    if (what) what[r] = kind[r];
  }
  const int all = count < 0 ? 0 : (count > out_cap ? out_cap : count);
  for (int r = m; r < all; ++r) {                                      /* beyond the 64 that count: as they are */
    const yf_track_info t = info[r];
    info_out[r] = t;
    if (what) what[r] = 0;
  }
  if (status) *status = bits;
}

/* a call behind its check, on host memory: stream by stream, step by step.  Returns n */
static inline long yfi_reid_run(const void* info, const void* out_counts, const void* desc, int out_cap, long streams, long steps, int layout,
                                const yf_reid_params* p, void* state, void* info_out, int32_t* what, int32_t* status) {
  for (long s = 0; s < streams; ++s)
    for (long t = 0; t < steps; ++t) {
      const long f = layout == YF_TRACK_TIME_MAJOR ? t * streams + s : s * steps + t;
      const size_t at = (size_t)f * (size_t)out_cap;
      yfi_reid_step((yf_reid_state*)state + s, (const yf_track_info*)info + at, (const yf_face_desc*)desc + at, ((const int32_t*)out_counts)[f],
                    out_cap, p, (yf_track_info*)info_out + at, what ? what + at : NULL, status ? status + f : NULL);
    }
  return streams * steps;
}

/* what the host can see of a call's arguments, in the order the entry points check them; NULL, or the text of the first fault */
static inline const char* yfi_reid_check(const void* info, const void* out_counts, const void* desc, int out_cap, long streams, long steps,
                                         int layout, const yf_reid_params* p, const void* state, const void* info_out, const void* what,
                                         const void* status) {
  if (!info || !out_counts || !desc || !p || !state || !info_out) return "d_info, d_out_counts, d_desc, params, d_state or d_info_out is NULL";
  if ((((uintptr_t)info | (uintptr_t)out_counts | (uintptr_t)desc | (uintptr_t)info_out | (uintptr_t)what | (uintptr_t)status) & 3) != 0)
    return "d_info, d_out_counts, d_desc, d_info_out, d_what and d_status must be 4-byte aligned";
  if (((uintptr_t)state & 7) != 0) return "d_state must be 8-byte aligned";
  if (out_cap < 1) return "out_cap must be >= 1";
  if (p->max_distance < 0) return "max_distance must be >= 0";
  if (p->max_age < 0) return "max_age must be >= 0";
  if (p->blend < 0 || p->blend > 256) return "blend must be in [0, 256]";
  if (layout != YF_TRACK_TIME_MAJOR && layout != YF_TRACK_STREAM_MAJOR) return "layout must be YF_TRACK_TIME_MAJOR or YF_TRACK_STREAM_MAJOR";
  if (streams < 0 || steps < 0) return "streams and steps must be >= 0";
  if (streams > 0 && steps > 2147483646l / streams) return "streams * steps must be in [0, 2^31 - 2]";
  return NULL;
}

#endif
