/* dlimgedit C ABI -- MI355X (gfx950) build.
 *
 * Binary-compatible replacement for the table exported by the reference library
 * (reference: src/include/dlimgedit/detail/dlimgedit.h:27-70, filled in src/dlimgedit.cpp:100-117).
 * The first 13 slots of dlimg_Api have the reference's order, signatures and POD layouts, so a
 * consumer compiled against the reference header (or its header-only C++ wrapper) can load this
 * library unchanged.  Slots after `last_error` are additions of this build (batch entry points,
 * SURVEY.md D5); a consumer that does not know them simply never reads past slot 13.
 *
 * Behaviour that differs from the reference, by design:
 *   - dlimg_gpu means "HIP device (MI355X)"; dlimg_cpu is reported as unsupported: this build has
 *     no CPU execution path (the onnxruntime CPU provider is not reproduced).
 *   - last_error() is per calling thread (the reference's global string is unsynchronised).
 *   - segment_objects returns dlimg_error (the BiRefNet graph is not part of this build); load_image reads PNG and
 *     JPEG files on the host, save_image writes PNG.
 *   - unlike the reference header this file is valid C (the struct tag is typedef'ed).
 */
#ifndef DLIMGEDIT_H_
#define DLIMGEDIT_H_

#include <stdint.h>

#if defined(_MSC_VER)
#    if defined(DLIMGEDIT_EXPORTS)
#        define DLIMG_API __declspec(dllexport)
#    else
#        define DLIMG_API __declspec(dllimport)
#    endif
#elif defined(DLIMGEDIT_EXPORTS)
#    define DLIMG_API __attribute__((visibility("default")))
#else
#    define DLIMG_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Opaque handles.  An environment must outlive every segmentation created from it. */
typedef struct dlimg_Environment_* dlimg_Environment;
typedef struct dlimg_Segmentation_* dlimg_Segmentation;

/* Borrowed view of 8-bit pixels, rows top to bottom.  24 bytes:
 * width@0 height@4 channels@8 stride@12 pixels@16.
 * channels: 1 mask, 3 rgb, 4 rgba, 5 bgra, 6 argb (5 and 6 are 4-byte pixels). stride is in bytes. */
typedef struct dlimg_ImageView {
    int width;
    int height;
    int channels;
    int stride;
    uint8_t* pixels;
} dlimg_ImageView;

typedef enum dlimg_Backend { dlimg_cpu = 0, dlimg_gpu = 1 } dlimg_Backend;

/* 16 bytes: backend@0, model_directory@8.  Weights are looked up as
 * <model_directory>/segmentation/sam_<variant>.dlw */
typedef struct dlimg_Options {
    dlimg_Backend backend;
    char const* model_directory;
} dlimg_Options;

typedef enum dlimg_Result { dlimg_success = 0, dlimg_error = 1 } dlimg_Result;

typedef struct dlimg_Api {
    /* ---- slots 0..12: identical to the reference ------------------------------------------ */

    /* 1 if the backend can be used on this machine; never fails. */
    int (*is_backend_supported)(dlimg_Backend);

    dlimg_Result (*create_environment)(dlimg_Environment* out_env, dlimg_Options const* options);
    void (*destroy_environment)(dlimg_Environment);

    /* Encodes one image.  *out_seg is assigned before encoding starts, so on dlimg_error the
     * caller still owns a handle and must destroy it.  Pixels are only read during the call.
     * The call returns once the pixels have been taken and the encoder pass is enqueued; the first call that needs
     * the embedding (get_segmentation_mask, ...) waits for it, and reports a pass that produced non-finite values
     * (DLIMGEDIT_SYNC_PROCESS=1: this call waits itself, as the reference's does). */
    dlimg_Result (*process_image_for_segmentation)(dlimg_Segmentation* out_seg, dlimg_ImageView const* image,
                                                   dlimg_Environment env);

    /* Exactly one of point {x,y} / region {x0,y0,x1,y1} is non-null (original image pixels).
     * out_masks[1] == NULL: single-mask mode, writes out_masks[0] only, out_accuracy untouched.
     * otherwise: writes three masks (decoder outputs 1..3) and their predicted IoU.
     * Each mask buffer is caller-allocated, width*height bytes, values 0 / 255. */
    dlimg_Result (*get_segmentation_mask)(dlimg_Segmentation seg, int const* point, int const* region,
                                          uint8_t** out_masks, float* out_accuracy);

    /* out_extent[0] = width, out_extent[1] = height of the image given to process. */
    void (*get_segmentation_extent)(dlimg_Segmentation seg, int* out_extent);
    void (*destroy_segmentation)(dlimg_Segmentation);

    dlimg_Result (*segment_objects)(dlimg_ImageView const* image, uint8_t* out_mask, dlimg_Environment env);

    dlimg_Result (*load_image)(char const* filepath, int* out_extent, int* out_channels, uint8_t** out_pixels);
    dlimg_Result (*save_image)(dlimg_ImageView const* image, char const* filepath);

    /* w*h*channels uninitialised bytes; release with destroy_image.  Once a GPU environment exists in the process this
     * memory (and load_image's) is pinned: images that lie in it are uploaded from where they lie, masks whose buffer
     * lies in it are written in place by the GPU.  destroy_image ignores foreign pointers. */
    uint8_t* (*create_image)(int width, int height, int channels);
    void (*destroy_image)(uint8_t const* pixels);

    /* Message of the most recent dlimg_error on the calling thread; valid until its next error. */
    char const* (*last_error)(void);

    /* ---- slots 13..: additions of the MI355X build ---------------------------------------- */

    /* Encodes `count` independent images in one batched pass.  out_segs[i] is assigned for every i
     * before any work starts (same ownership rule as the single-image call). */
    dlimg_Result (*process_images_for_segmentation)(dlimg_Segmentation* out_segs, dlimg_ImageView const* images,
                                                    int count, dlimg_Environment env);

    /* One single-mask query per entry, decoded as one batch.  points: count x {x,y} or NULL;
     * regions: count x {x0,y0,x1,y1} or NULL (at least one of them non-null).  One array: entry i is a point
     * or a box query, as get_segmentation_mask.  Both arrays: entry i is the box regions[i] refined by the
     * foreground point points[i] -- SAM's combined prompt (point, top-left, bottom-right; labels 1, 2, 3; no
     * padding point), whose single mask is the decoder's output 0.  [get_segmentation_mask keeps the
     * reference's rule: given both, the point wins and the region is ignored.]  The same handle may
     * appear several times (several prompts on one cached embedding). out_masks[i]: width*height bytes.
     * Several clicks per prompt: an entry whose segs[i] is NULL is a continuation entry -- points[i] is one more
     * click of the prompt opened by the nearest entry with a handle in front of it, its label regions[4 i] (1
     * foreground, 0 background; the other three ints 0), foreground when regions is NULL.  The head entry is read
     * as above and its own click is a foreground click; in a call with continuation entries a head whose region
     * is empty (x1 < x0) has no box.  A prompt has at most 8 clicks and gets ONE mask, out_masks of its head (the
     * continuation entries' out_masks are not read and may be NULL).  Prompts of different sizes may share a call.
     * Refused: more than 8 clicks, a continuation entry in front, a label other than 0 / 1.
     * Refinement marks (SAM's mask input): a continuation entry whose four ints are {DLIMG_REFINE_MARK, 0, 0, 0} is a
     * mark, not a click -- points[i] is not read and it does not count towards the 8 clicks.  A prompt with m marks
     * is decoded in m + 1 stages on the GPU that holds the embedding: stage j takes the clicks in front of mark j
     * (the head's included), the last stage all clicks, every stage the prompt's box if it has one; from the second
     * stage on a stage takes the low-res logits of the stage before it as its mask input, the way SAM's interactive
     * predictor feeds them back.  The mask of the last stage is delivered.  Refused (the message names the mark): a
     * mark directly after a mark, a mark as the last entry of a prompt, a mark with non-zero trailing ints, a mark
     * for a model whose file has no mask branch (pe.mask.*).  A call without marks is read as it always was.
     * Clean-up marks (SAM's remove_small_regions): a continuation entry whose four ints are {DLIMG_CLEAN_MARK, max_hole,
     * max_island, 0} is neither a click nor a stage -- points[i] is not read and it does not count towards the 8 clicks.
     * The ONE mask its prompt delivers is cleaned on the GPU before it is copied out, thresholds in pixels of that mask,
     * 8-connectivity for both polarities: first every connected component of the background with fewer than max_hole
     * pixels becomes foreground (max_hole 0: skipped), then, on that result, every connected component of the foreground
     * with fewer than max_island pixels becomes background (max_island 0: skipped) -- except that when all components
     * are below max_island the largest one stays, and among equal largest the one whose first pixel in raster order comes
     * first (SAM leaves this tie to OpenCV's label numbering; the raster-order rule is this library's).  For a prompt
     * with refinement marks the mask of the last stage is cleaned; the logits fed back between stages are untouched.
     * A call with a clean-up mark needs `regions`, not `points`: a box-only call may clean its masks, and like every call
     * with continuation entries it reads an empty head region as "no box".  Refused (the message says "mark" and names
     * the entry): a clean-up mark that is not the last entry of its prompt (so at most one per prompt; a refinement mark
     * directly in front of it is still that prompt's last click-side entry and refused as such), one in front of any
     * head, a negative threshold, both thresholds 0, a non-zero fourth int, and a prompt left with neither a click nor a
     * box.  A call without clean-up marks is read as it always was.
     * Prior marks (a mask input supplied by the caller): a continuation entry whose four ints are {DLIMG_PRIOR_MARK,
     * strength_milli, 0, 0} DIRECTLY BEHIND ITS HEAD -- see DLIMG_PRIOR_MARK below.  It is the one continuation entry whose
     * out_masks[i] is READ: width * height bytes of the head's image, the prior.
     * Lasso marks (a selection snapped to the object): a continuation entry whose four ints are {DLIMG_LASSO_MARK,
     * strength_milli, what, 0} DIRECTLY BEHIND ITS HEAD -- see DLIMG_LASSO_MARK below.  Its out_masks[i] is READ likewise: the
     * selection, from which the prompt's box and first click are derived on the GPU.
     * Matte marks (an image-guided soft edge): a continuation entry whose four ints are {DLIMG_MATTE_MARK, radius, eps,
     * channels}, THE LAST ENTRY OF ITS PROMPT -- see DLIMG_MATTE_MARK below.  Its out_masks[i] is READ as well: the image, the
     * guide; the prompt's mask is then delivered as coverage 0 .. 255.
     * Stroke marks (clicks sampled from a scribble): a continuation entry whose four ints are {DLIMG_STROKE_MARK, clicks,
     * label, 0}, wherever a click entry may stand -- see DLIMG_STROKE_MARK below.  Its out_masks[i] is READ too: the stroke map,
     * from which that many clicks of that label are derived on the GPU.
     * Cut-out marks (a matte's foreground colours as RGBA): a continuation entry whose four ints are {DLIMG_CUTOUT_MARK,
     * radius, 0, 0} DIRECTLY BEHIND THE MATTE MARK, the last entry of its prompt then -- see DLIMG_CUTOUT_MARK below.  It is
     * the one continuation entry whose out_masks[i] is WRITTEN: height * width * 4 bytes.
     * Edge marks (grow, shrink, feather, border): a continuation entry whose four ints are {DLIMG_EDGE_MARK, offset, feather,
     * border}, behind the clicks and the clean-up mark of its prompt and in front of its matte mark -- see DLIMG_EDGE_MARK
     * below.  Its out_masks[i] is not read. */
    dlimg_Result (*get_segmentation_masks)(dlimg_Segmentation const* segs, int count, int const* points,
                                           int const* regions, uint8_t** out_masks);
} dlimg_Api;

/* regions[4 i] of a refinement mark in get_segmentation_masks (slot 14): the first value SAM's label space leaves
 * free (-1 padding point, 0 / 1 clicks, 2 / 3 box corners). */
#define DLIMG_REFINE_MARK 4
/* regions[4 i] of a clean-up mark in get_segmentation_masks (slot 14): {DLIMG_CLEAN_MARK, max_hole, max_island, 0}.
 * 5 stays what it was, a refused label. */
#define DLIMG_CLEAN_MARK 6
/* regions[4 i] of a grid mark in get_segmentation_masks (slot 14): {DLIMG_GRID_MARK, side, iou_permille,
 * stability_permille} turns its prompt into a grid prompt ("segment everything", SAM's automatic mask generator in a
 * narrow form).  A grid prompt is exactly two entries: the head (handle, out_masks of width * height bytes, an EMPTY region,
 * x1 < x0) and the mark; neither entry's point is read, and `points` may be NULL.  side is 1 .. 32; the two thresholds may
 * be any int, 0 meaning SAM's defaults 880 and 950.  out_masks[head] receives a LABEL MAP: 0 where no segment lies, k in
 * 1 .. 255 for the k-th kept segment.  The side * side points (i, j) at pixel (floor((2 i + 1) W / (2 side)),
 * floor((2 j + 1) H / (2 side))) are decoded as one-click prompts; the candidates are outputs 1 .. 3 of every prompt.  A
 * candidate is scored on its 256 x 256 low-resolution logits over the part that lies inside the image (x < ceil(pre_w / 4),
 * y < ceil(pre_h / 4), pre: the extent the image was encoded at; SAM scores at the original resolution): n_hi, n_mid, n_lo
 * logits > +1, > 0, > -1 and the box of the logits > 0.  It passes when n_mid > 0, n_lo > 0, its IoU prediction >=
 * iou_permille / 1000 (fp32) and n_hi * 1000 >= stability_permille * n_lo.  The passing candidates go through box NMS by IoU
 * prediction (ties: lower candidate index first; suppressed when inter * 10 > 7 * union with torchvision's box area on the
 * inclusive corners; at most 255 kept), the kept ones are labelled by n_mid descending (ties: NMS order), and a pixel
 * carries the largest label whose mask -- exactly the mask a single query would deliver for that output -- is 255 there:
 * the smallest segment lies on top.  Other prompts of the call may be anything the call takes.  Refused before anything is
 * launched (the message says "mark" and names the entry): side out of range, a non-empty head region, any further
 * continuation entry in the prompt (click, refinement mark, clean-up mark), a mark in front of any head.  A call without
 * grid marks is read as it always was. */
#define DLIMG_GRID_MARK 7
/* regions[4 i] of a prior mark in get_segmentation_masks (slot 14): {DLIMG_PRIOR_MARK, strength_milli, 0, 0} directly behind
 * its head hands the prompt a mask the caller already holds -- a lasso or brush selection, the mask of the last query -- as
 * SAM's mask input.  The mark is neither a click nor a stage; points[i] is not read and it does not count towards the 8
 * clicks.  out_masks[i] OF THE MARK IS READ AS THE PRIOR: width * height bytes of the head's image, tightly packed, values
 * 0 .. 255 read as coverage (soft selections count).  It may be the same memory as out_masks[head] -- a mask refined in
 * place: the prior is taken before anything is delivered.  A prior in memory from create_image is sent from where it lies.
 * On the GPU the prior becomes the 256 x 256 plane of the prompt encoder's mask branch: a low-res pixel is the mean coverage
 * of the source pixels it stands for, mapped from 0 .. 255 to -1 .. +1 and multiplied by strength_milli / 1000; what lies
 * outside the image is background (-strength).  strength_milli is 1 .. 100000; 0 means 8000, a choice and not a
 * measurement: this library was built and tested with synthetic weights, and SAM's own logits of a confident mask are of
 * that order.  The plane is the mask input of the prompt's FIRST stage; a prompt with refinement marks feeds its later
 * stages as before, a clean-up mark cleans the delivered mask as before, and the prompt-size limits are unchanged.  Like
 * every call with continuation entries the call needs `regions`, an empty head region means "no box", and the prompt must
 * still hold a click or a box (a box alone, without `points`, will do).  Refused before anything is launched (the message
 * says "mark" and names the entry): a mark that is not directly behind a head, a NULL prior, a negative strength or one
 * above 100000, non-zero trailing ints, a second prior mark on the same prompt, a model whose file has no mask branch
 * (pe.mask.*), a grid prompt, and dlimg_amd_get_segmentation_masks_device, which has no per-entry pointer to read a prior
 * from.  A call without prior marks is read as it always was. */
#define DLIMG_PRIOR_MARK 8
/* regions[4 i] of a lasso mark in get_segmentation_masks (slot 14): {DLIMG_LASSO_MARK, strength_milli, what, 0} directly behind
 * its head makes a prompt of a selection the caller already holds -- a dragged lasso, a painted blob -- so that it snaps to the
 * object.  points[i] of the mark is not read.  out_masks[i] OF THE MARK IS READ AS THE SELECTION under the rules of a prior
 * mark: width * height bytes of the head's image, tightly packed, 0 .. 255 read as coverage; it may be out_masks[head] itself
 * (it is taken before anything is delivered); in memory from create_image it is sent from where it lies.
 * what is a bit set, 0 meaning all three:
 *   DLIMG_LASSO_BOX    the prompt's box is the selection's box; the head's region must be empty (x1 < x0)
 *   DLIMG_LASSO_CLICK  the prompt's FIRST click is a foreground click at the selection's most interior point; it counts towards
 *                      the 8 clicks and towards a SAM-HQ file's point limit
 *   DLIMG_LASSO_MASK   the selection is also the mask input of the prompt's first stage, exactly as a prior mark with this
 *                      strength_milli would make it (0 = 8000; needs pe.mask.*)
 * strength_milli is 0 without DLIMG_LASSO_MASK.  what == 4 derives nothing and is refused: that is a prior mark.
 * The derivation is integer arithmetic on the 256 x 256 low-res grid of the prior plane.  A cell is INSIDE when the mean
 * coverage of the source pixels it stands for is above one half (where the prior plane is positive); everything else,
 * everything outside the image included, is background.  The box is the union of the inside cells' source pixels, {x0, y0, x1,
 * y1} with x1, y1 one past the last pixel.  The click is the middle pixel of the inside cell farthest (exact Euclidean distance
 * on the grid) from any background cell, ties to the smallest y, then the smallest x.
 * The packed order is SAM's: the derived click, the caller's clicks in the order given (the head's point is the first of them
 * in a call with `points`), the box corners; the padding point only without a box.  Refinement marks, a clean-up mark and
 * further clicks work as on any prompt: the derived click belongs to the first stage, the box to every stage.  A lasso-only
 * prompt lives in a call without `points`, like a box-only call: head {0, 0, -1, -1}, then the mark.
 * Refused before anything is launched (the message says "mark" and names the entry): a mark that is not directly behind a
 * head, a second lasso mark or a prior mark on the same prompt, a NULL selection, what outside 0 .. 7, what == 4, a non-zero
 * fourth int, strength_milli outside 0 .. 100000 or non-zero without DLIMG_LASSO_MASK, DLIMG_LASSO_BOX on a head whose region
 * is not empty, DLIMG_LASSO_MASK on a model without the mask branch, a grid prompt, more than 8 clicks counting the derived
 * one, and dlimg_amd_get_segmentation_masks_device, which has no per-entry pointer to read a selection from.
 * ONE refusal arrives later: a selection with no inside cell (all of it below half coverage of every low-res cell) is
 * reported after its derivation ran and before its prompt is decoded -- "entry i: the lasso mark's selection is empty ...".
 * out_masks of that prompt is not written; what OTHER prompts of the same call have received by then is unspecified, as with
 * the report of an encoder overflow.  The call waits for the GPU once per lasso prompt (the derived prompt comes back to the
 * host).  A call without lasso marks is read as it always was. */
#define DLIMG_LASSO_MARK 10
#define DLIMG_LASSO_BOX 1
#define DLIMG_LASSO_CLICK 2
#define DLIMG_LASSO_MASK 4
/* regions[4 i] of a matte mark in get_segmentation_masks (slot 14): {DLIMG_MATTE_MARK, radius, eps, channels}, THE LAST ENTRY
 * OF ITS PROMPT (behind the clean-up mark when the prompt has one, which is then the last of the remaining entries, as it must
 * be), makes the prompt deliver its one mask as COVERAGE 0 .. 255 instead of 0 / 255: the mask the same prompt would deliver
 * without the mark (after clean-up, if it has a clean-up mark), filtered with He et al.'s guided filter, the guide being the
 * grey image.  Hair, fur and every edge that runs between the 256 x 256 low-res cells then follow the picture.
 * The mark is neither a click nor a stage; points[i] is not read and it does not count towards the 8 clicks.  out_masks[i] OF
 * THE MARK IS READ AS THE GUIDE: the image the head's handle was made from, height * width * channels bytes, tightly packed.
 * It is uploaded before the mask of its prompt is delivered; in memory from create_image / load_image it is sent from where
 * it lies.  channels is 1, 3 or 4; grey G = the byte for 1, else (c0 + 2 c1 + c2 + 2) >> 2, so RGBA and BGRA give the same
 * matte and a fourth channel is ignored.  radius is 1 .. 32 pixels of the image.  eps is 1 .. 65025, in squared grey levels of
 * the 0 .. 255 scale; 0 means 650, about 0.01 on the unit scale -- a choice, not a measurement.
 * The definition is integer arithmetic, so the bytes are the same wherever they are computed.  With p the mask, F = 16,
 * win(x, y) the (2 radius + 1)^2 square around a pixel clipped to the image, N its pixel count, fdiv floor division:
 *   S_G, S_p, S_GG, S_Gp = sums of G, p, G^2, G p over win(x, y)
 *   cov = N S_Gp - S_G S_p      den = N S_GG - S_G^2 + eps N^2
 *   A = fdiv(2 cov 2^F + den, 2 den)      B = fdiv(2 (S_p 2^F - A S_G) + N, 2 N)
 *   S_A, S_B = sums of A, B over win(x, y)
 *   out = clamp(fdiv(2 (S_A G(x, y) + S_B) + N 2^F, 2 N 2^F), 0, 255)
 * which is within one grey level of the float64 filter.  Where the mask is one value over the radius-2r square around a pixel
 * the pixel keeps it exactly; with a constant guide the matte is the twice box-filtered mask.
 * Everything in front of the mark is read as ever: clicks, box, refinement, prior, lasso and clean-up marks, SAM-HQ models.
 * Like every call with continuation entries the call needs `regions`, and an empty head region means "no box".
 * Refused before anything is launched (the message says "mark" and names the entry): a matte mark that is not the last entry
 * of its prompt, one in front of any head, a second one on a prompt, a NULL guide, radius outside 1 .. 32, eps outside
 * 0 .. 65025, channels other than 1 / 3 / 4, a grid prompt (a label map is not a coverage), and
 * dlimg_amd_get_segmentation_masks_device, which has no per-entry pointer to read a guide from.  A call without matte marks
 * is read as it always was. */
#define DLIMG_MATTE_MARK 11      /* 5 and 9 stay refused labels */
/* regions[4 i] of a stroke mark in get_segmentation_masks (slot 14): {DLIMG_STROKE_MARK, clicks, label, 0} makes clicks of a
 * scribble the caller holds -- a foreground stroke drawn over the object, a background stroke over what the selection must
 * leave out.  label is 1 (foreground) or 0 (background); clicks is 1 .. 8, 0 meaning 3 -- a choice, not a measurement.
 * points[i] of the mark is not read.  out_masks[i] OF THE MARK IS READ AS THE STROKE MAP: width * height bytes of the head's
 * image, tightly packed; a pixel belongs to the stroke when its byte is >= 128.  The map is taken before anything is delivered
 * (it may be out_masks[head] itself); in memory from create_image it is sent from where it lies.
 * The mark may stand wherever a click entry may stand and STANDS FOR `clicks` click entries of its label at that position: they
 * count towards the 8 clicks and towards a SAM-HQ file's point limit, a refinement mark behind them stages them like any click,
 * and a prompt may hold several stroke marks (stroke, refinement mark, stroke).  Prior and lasso marks keep their place directly
 * behind the head, in front of every stroke mark; clean-up and matte marks stay last, behind every stroke mark.  In a call
 * WITHOUT `points` the first foreground click a prompt's strokes stand for takes the place of the head's own click, the others
 * keep their order; every prompt of such a call therefore needs a foreground stroke mark, and a click entry still needs
 * `points`.  With `points` the head's click comes first, as always.
 * The derivation is integer arithmetic on the 256 x 256 low-res grid.  With the image encoded at pre_w x pre_h, cell (x, y),
 * x < ceil(pre_w / 4), y < ceil(pre_h / 4), stands for the source pixels floor(4 x W / pre_w) .. ceil(min(4 x + 4, pre_w) W /
 * pre_w) - 1 (rows likewise), exactly as for a prior mark, and is ON when ANY of them belongs to the stroke (a maximum, not the
 * prior's mean: a one-pixel line switches on every cell it crosses).  With n ON cells of coordinate sums Sx, Sy the first click
 * is the ON cell with the smallest (n x - Sx)^2 + (n y - Sy)^2 -- the one nearest the centroid; every further click is the ON
 * cell with the largest minimum of dx^2 + dy^2 to the cells chosen before it (farthest-point sampling).  Ties go to the smallest
 * y, then the smallest x; with fewer ON cells than clicks a cell is chosen again.  A click is the middle pixel of its cell's
 * source pixels.
 * Refused before anything is launched (the message says "mark" and names the entry): a non-zero fourth int, label outside
 * {0, 1}, clicks outside 0 .. 8, a NULL map, a mark in front of any head, a grid prompt, a stroke mark in front of a prior or
 * lasso mark or behind a clean-up or matte mark, a call without `points` in which a prompt has no foreground stroke mark
 * (background strokes alone are no prompt), more than 8 clicks or a SAM-HQ file's limit counting the derived clicks, and
 * dlimg_amd_get_segmentation_masks_device, which has no per-entry pointer to read a map from.
 * ONE refusal arrives later, as a lasso mark's: a map without a stroke pixel in the image is reported after the derivation ran
 * and before its prompt is decoded -- "entry i: the stroke mark's map is empty ...".  out_masks of that prompt is not written;
 * what OTHER prompts of the same call have received by then is unspecified.  The call waits for the GPU once per prompt with
 * stroke marks, however many it has.  A call without stroke marks is read as it always was. */
#define DLIMG_STROKE_MARK 12
/* regions[4 i] of a cut-out mark in get_segmentation_masks (slot 14): {DLIMG_CUTOUT_MARK, radius, 0, 0} DIRECTLY BEHIND THE
 * MATTE MARK OF ITS PROMPT, and then the last entry of the prompt, cuts the object out: inside the soft band a pixel of the
 * image is a mix of foreground and background colour, and multiplying it by the coverage carries the old background along as a
 * fringe.  The mark estimates the FOREGROUND colour of every pixel (one pass of Forte's Blur-Fusion) from the matte mark's guide
 * -- so that mark's channels is 3 or 4 -- and the coverage the prompt delivers.
 * The mark is neither a click nor a stage; points[i] is not read and it does not count towards the 8 clicks.  out_masks[i] OF
 * THE MARK IS WRITTEN: it receives height * width * 4 bytes, tightly packed.  Bytes 0 .. 2 of a pixel are the estimated
 * foreground colour in the channel order of the guide's first three channels (RGBA in gives RGBA out, BGRA in gives BGRA out),
 * byte 3 is the coverage.  out_masks[head] still receives the coverage, byte for byte what the same prompt delivers without
 * the cut-out mark.  The pointer may be the guide itself when channels is 4: the image is then decontaminated in place, its
 * fourth byte replaced by the coverage (the guide is taken before anything is delivered).  In memory from create_image the
 * result is copied in place by the GPU's copy engine; otherwise it goes through pinned staging of its own size.  The prompt
 * costs no further wait for the GPU: everything runs in stream order behind the matte.
 * radius is 1 .. 32 pixels of the image; 0 means 16, a choice and not a measurement.
 * The definition is integer arithmetic, so the bytes are the same wherever they are computed.  With a the delivered coverage,
 * I_c channel c of the guide (c = 0, 1, 2), win(x, y) the (2 radius + 1)^2 square around a pixel clipped to the image, N its
 * pixel count, fdiv floor division:
 *   S_a, S_I, S_Ia = sums of a, I_c, I_c a over win(x, y)         S_b = 255 N - S_a       S_Ib = 255 S_I - S_Ia
 *   Fh = fdiv(512 S_Ia + S_a, 2 S_a) if S_a > 0, else 256 I_c(x, y)
 *   Bh = fdiv(512 S_Ib + S_b, 2 S_b) if S_b > 0, else 256 I_c(x, y)
 *   num = 65025 Fh + a (65280 I_c - a Fh - (255 - a) Bh)          D = 65025 * 256
 *   out_c = clamp(fdiv(2 num + D, 2 D), 0, 255)                   out_3 = a
 * which is within one level of the float64 Blur-Fusion.  Where a == 255 the pixel keeps its colour exactly; a constant image
 * stays constant; where no pixel of the window is covered the colour is the image's; a fully transparent pixel near the object
 * carries the neighbouring foreground's colour, which is what straight-alpha compositing and later resampling want.
 * Refused before anything is launched (the message says "mark" and names the entry): a cut-out mark that is not directly
 * behind a matte mark, one that is not the last entry of its prompt, a second one on a prompt, a matte mark with channels == 1
 * in front of it, a NULL pointer, a pointer equal to out_masks[head], radius outside 0 .. 32, non-zero trailing ints, a mark
 * in front of any head, and dlimg_amd_get_segmentation_masks_device, which has no per-entry pointer to write to.  A grid
 * prompt is refused through its matte mark.  A call without cut-out marks is read as it always was. */
#define DLIMG_CUTOUT_MARK 13
/* regions[4 i] of an edge mark in get_segmentation_masks (slot 14): {DLIMG_EDGE_MARK, offset, feather, border} grows, shrinks,
 * feathers or borders the mask its prompt delivers -- the four of an editor's Select > Modify menu -- on the GPU, in front of
 * the copy.  The mark is neither a click nor a stage; points[i] and out_masks[i] of the mark are not read and it does not count
 * towards the 8 clicks.  A prompt has one at most.  It stands behind every click, stroke mark and refinement mark of its prompt
 * and behind the clean-up mark when there is one; in front of the matte mark (and with it the cut-out mark) when there is one,
 * and is otherwise the last entry of its prompt.  The stages run in that order: clean-up, edge, matte, cut-out; the matte
 * filters what the edge mark delivered.
 * offset is -64 .. 64 pixels (positive grows, negative shrinks), feather 0 .. 32, border 0 .. 32; not all three 0.
 * The definition is integer arithmetic, so the bytes are the same wherever they are computed.  A pixel of the mask is
 * foreground when its byte is >= 128.  Pixels outside the image do not exist: they are neither foreground nor background, so
 * a mask that touches the image's edge is not eroded from it.  d2 of a pixel is the exact squared Euclidean distance to the
 * nearest pixel of the other kind, infinite where the image has none.  With isqrt rounding down and fdiv floor division:
 *   q = isqrt(65536 d2)                   the distance in 1/256 pixel
 *   S = q - 128 for a foreground pixel, -(q - 128) for a background pixel        (the edge runs half-way between pixel centres)
 *   T = S + 256 offset;                   border > 0:  T <- 256 border - |T|     (a band of `border` pixels either side)
 *   out = 255 if T > 0 else 0                                                    (feather == 0)
 *   out = clamp(fdiv(255 (T + 256 f) + 256 f, 512 f), 0, 255)                    (feather == f > 0: a ramp 2 f pixels wide)
 * With R = |offset| + feather + border + 1 every d2 >= R^2, the infinite one included, gives the byte of d2 == R^2.  With
 * feather == border == 0 this is binary dilation or erosion by the disc {(dx, dy): isqrt(65536 (dx^2 + dy^2)) < 256 |offset| +
 * 128}: 3 x 3 for 1, the 21-pixel disc for 2; no distance sits on a tie, so the two are exact duals.
 * The prompt costs no further wait for the GPU: the kernels run in stream order behind the post-processing, in place where the
 * mask is delivered into memory of the producing GPU, else in staging.
 * Refused before anything is launched (the message says "mark" and names the entry): values outside these ranges, all three
 * 0 (the identity), a second edge mark on a prompt, a mark in front of any head, a mark in front of a click, stroke,
 * refinement or clean-up mark or behind a matte mark, and an edge mark on a grid prompt (a label map has no edge to move).  A
 * call without edge marks is read as it always was. */
#define DLIMG_EDGE_MARK 14

/* The only exported symbol of the drop-in ABI.  Returns a process-lifetime table; idempotent. */
DLIMG_API dlimg_Api const* dlimg_init(void);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* DLIMGEDIT_H_ */
