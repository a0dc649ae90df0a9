// dlimgedit.hpp -- C++ convenience layer over the C-ABI of the MI355X build (single header).
//
// Source-compatible with the consumer-facing API of the reference's wrapper
// (reference: src/include/dlimgedit/dlimgedit.hpp:16-191): namespace dlimg, Extent / Channels /
// ImageView / Image, Backend / Options / Environment, Point / Region / Segmentation (process,
// compute_mask, compute_masks, extent), segment_objects, initialize, Exception.  Code written
// against the reference's header compiles against this one; binaries built against the reference's
// header need no rebuild at all because the C table underneath is layout-identical.
//
// Additions: Segmentation::process_batch and Segmentation::compute_mask_batch (batched entry
// points of this build), Click and the compute_mask / compute_mask_batch forms that take several clicks per prompt.  Requires C++17.  Define DLIMGEDIT_LOAD_DYNAMIC before including to bind
// the library at run time: dlsym "dlimg_init" yourself and pass the result to dlimg::initialize().
#pragma once

#include "dlimgedit.h"

#include <algorithm>
#include <array>
#include <cstddef>
#include <exception>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <vector>
#ifndef DLIMGEDIT_NO_FILESYSTEM
#    include <filesystem>
#endif

namespace dlimg {

// ---------------------------------------------------------------------------------------------
// binding to the C table

namespace detail {
inline dlimg_Api const*& table() {
    static dlimg_Api const* t = nullptr;
    return t;
}
}  // namespace detail

#ifdef DLIMGEDIT_LOAD_DYNAMIC
inline void initialize(dlimg_Api const* api) { detail::table() = api; }
#else
inline void initialize(dlimg_Api const* api = dlimg_init()) { detail::table() = api; }
#endif

inline dlimg_Api const& api() {
#ifndef DLIMGEDIT_LOAD_DYNAMIC
    if (!detail::table()) detail::table() = dlimg_init();
#endif
    return *detail::table();
}

class Exception : public std::exception {
  public:
    explicit Exception(std::string message) : message_(std::move(message)) {}
    char const* what() const noexcept override { return message_.c_str(); }

  private:
    std::string message_;
};

namespace detail {
inline void check(dlimg_Result r) {
    if (r != dlimg_success) throw Exception(api().last_error());
}
}  // namespace detail

// ---------------------------------------------------------------------------------------------
// images

struct Extent {
    int width = 0;
    int height = 0;
};
constexpr bool operator==(Extent a, Extent b) { return a.width == b.width && a.height == b.height; }
constexpr bool operator!=(Extent a, Extent b) { return !(a == b); }

// One byte per channel; bgra and argb are four-byte pixels.
enum class Channels { mask = 1, rgb = 3, rgba = 4, bgra, argb };
constexpr int count(Channels c) { return static_cast<int>(c) > 4 ? 4 : static_cast<int>(c); }

class Image;

// Borrowed pixels, row-major, origin top-left.  Same 24-byte layout as dlimg_ImageView.
struct ImageView {
    Extent extent;
    Channels channels = Channels::rgba;
    int stride = 0;  // bytes per row
    uint8_t const* pixels = nullptr;

    ImageView() noexcept = default;
    ImageView(uint8_t const* data, Extent e, Channels c = Channels::rgba) noexcept
        : extent(e), channels(c), stride(e.width * count(c)), pixels(data) {}
    ImageView(Image const& image) noexcept;
};
static_assert(sizeof(ImageView) == sizeof(dlimg_ImageView), "ImageView must mirror dlimg_ImageView");

// Owning, tightly packed pixels allocated by the library.
class Image {
  public:
    explicit Image(Extent e, Channels c = Channels::rgba)
        : extent_(e), channels_(c), pixels_(api().create_image(e.width, e.height, count(c))) {}
    Image(Image&& o) noexcept : extent_(o.extent_), channels_(o.channels_), pixels_(std::exchange(o.pixels_, nullptr)) {}
    Image& operator=(Image&& o) noexcept {
        std::swap(extent_, o.extent_);
        std::swap(channels_, o.channels_);
        std::swap(pixels_, o.pixels_);
        return *this;
    }
    Image(Image const&) = delete;
    Image& operator=(Image const&) = delete;
    ~Image() {
        if (pixels_) api().destroy_image(pixels_);
    }

    Extent extent() const noexcept { return extent_; }
    Channels channels() const noexcept { return channels_; }
    uint8_t* pixels() noexcept { return pixels_; }
    uint8_t const* pixels() const noexcept { return pixels_; }
    size_t size() const noexcept { return size_t(extent_.width) * extent_.height * count(channels_); }

    static Image load(char const* filepath) {
        uint8_t* px = nullptr;
        Extent e;
        int c = 0;
        detail::check(api().load_image(filepath, &e.width, &c, &px));
        return Image(e, static_cast<Channels>(c), px);
    }
    static void save(ImageView const& image, char const* filepath) {
        detail::check(api().save_image(reinterpret_cast<dlimg_ImageView const*>(&image), filepath));
    }
#ifndef DLIMGEDIT_NO_FILESYSTEM
    static Image load(std::filesystem::path const& p) { return load(p.string().c_str()); }
    static void save(ImageView const& image, std::filesystem::path const& p) { save(image, p.string().c_str()); }
#endif

  private:
    Image(Extent e, Channels c, uint8_t* adopted) : extent_(e), channels_(c), pixels_(adopted) {}
    Extent extent_;
    Channels channels_;
    uint8_t* pixels_ = nullptr;
};

inline ImageView::ImageView(Image const& image) noexcept
    : extent(image.extent()), channels(image.channels()), stride(extent.width * count(channels)), pixels(image.pixels()) {}

// ---------------------------------------------------------------------------------------------
// environment

enum class Backend { cpu, gpu };   // gpu = HIP device (MI355X); cpu is not available in this build

struct Options {
    Backend backend = Backend::cpu;
    char const* model_directory = "models";   // holds segmentation/sam_<variant>.dlw
};
static_assert(sizeof(Options) == sizeof(dlimg_Options), "Options must mirror dlimg_Options");

namespace detail {
struct EnvDeleter { void operator()(dlimg_Environment_* h) const { api().destroy_environment(h); } };
struct SegDeleter { void operator()(dlimg_Segmentation_* h) const { api().destroy_segmentation(h); } };
}  // namespace detail

// Owns the model cache; thread-safe; must outlive every Segmentation created from it.
class Environment {
  public:
    static bool is_supported(Backend b) noexcept { return api().is_backend_supported(dlimg_Backend(int(b))) != 0; }

    explicit Environment(Options const& options = {}) {
        dlimg_Environment h = nullptr;
        detail::check(api().create_environment(&h, reinterpret_cast<dlimg_Options const*>(&options)));
        handle_.reset(h);
    }
    Environment(std::nullptr_t) noexcept {}

    dlimg_Environment handle() const noexcept { return handle_.get(); }
    explicit operator bool() const noexcept { return bool(handle_); }

  private:
    std::unique_ptr<dlimg_Environment_, detail::EnvDeleter> handle_;
};

// ---------------------------------------------------------------------------------------------
// segmentation

struct Point {
    int x = 0;
    int y = 0;
};
constexpr bool operator==(Point a, Point b) { return a.x == b.x && a.y == b.y; }
constexpr bool operator!=(Point a, Point b) { return !(a == b); }

struct Region {
    Point top_left;
    Point bottom_right;

    constexpr Region() = default;
    constexpr Region(Point tl, Point br) : top_left(tl), bottom_right(br) {}
    constexpr Region(Point origin, Extent e) : top_left(origin), bottom_right{origin.x + e.width, origin.y + e.height} {}
    constexpr Extent extent() const { return Extent{bottom_right.x - top_left.x, bottom_right.y - top_left.y}; }
};
constexpr bool operator==(Region a, Region b) { return a.top_left == b.top_left && a.bottom_right == b.bottom_right; }
constexpr bool operator!=(Region a, Region b) { return !(a == b); }

// Clean-up of a delivered mask (SAM's remove_small_regions, on the GPU): background components below max_hole pixels are
// filled, then foreground components below max_island pixels dropped (8-connectivity; 0 skips a step; when every island is
// below max_island the largest stays, the first in raster order among equals).  Travels as a clean-up mark of table slot 14.
struct MaskCleanup {
    int max_hole = 0, max_island = 0;
};

// "Segment everything": a side x side grid of point prompts (1 .. 32), the candidates kept whose predicted IoU is at least
// iou_permille / 1000 and whose stability is at least stability_permille / 1000 (0: SAM's defaults, 880 and 950).  Travels
// as a grid mark of table slot 14.
struct GridOptions {
    int side = 32, iou_permille = 0, stability_permille = 0;
};

// A prior: a mask the caller already holds (a lasso or brush selection, the mask of the last query) as SAM's mask input of a
// click-to-refine prompt.  mask: width * height bytes of the segmentation's image, tightly packed, 0 .. 255 read as coverage
// (soft selections count); it may be the memory the result goes to.  strength_milli: 1 .. 100000, the logit a fully covered
// pixel stands for, in thousandths; 0: the library's default, 8000.  Travels as a prior mark of table slot 14 (dlimgedit.h,
// DLIMG_PRIOR_MARK).  Needs a model with the mask branch.
struct Prior {
    uint8_t const* mask = nullptr;
    int strength_milli = 0;
};

// A lasso: a selection the caller already holds (a dragged lasso, a painted blob) that should SNAP to the object.  mask: as a
// Prior's.  what: a bit set of DLIMG_LASSO_BOX (the prompt's box is the selection's), DLIMG_LASSO_CLICK (the prompt's first
// click is a foreground click at the selection's most interior point) and DLIMG_LASSO_MASK (the selection is the mask input of
// the first stage as well, at strength_milli as a Prior's; needs a model with the mask branch); 0: all three.  Box and click
// are derived on the GPU.  strength_milli is 0 without DLIMG_LASSO_MASK.  Travels as a lasso mark of table slot 14
// (dlimgedit.h, DLIMG_LASSO_MARK).
struct Lasso {
    uint8_t const* mask = nullptr;
    int what = 0;
    int strength_milli = 0;
};

// A matte: the prompt's mask delivered as COVERAGE 0 .. 255 with an edge that follows the picture (He et al.'s guided filter on
// the GPU, in integers; dlimgedit.h, DLIMG_MATTE_MARK).  guide: the image the segmentation was made from, height * width *
// channels bytes, tightly packed; channels 1, 3 or 4 (RGBA and BGRA give the same matte).  radius: 1 .. 32 pixels.  eps: 1 ..
// 65025 squared grey levels; 0: the library's default, 650.  Travels as a matte mark of table slot 14, the last entry of its
// prompt.
struct Matte {
    uint8_t const* guide = nullptr;
    int channels = 4;
    int radius = 8;
    int eps = 0;
};

// A stroke: a scribble the caller holds, from which `clicks` clicks of one label are sampled on the GPU -- spread along it:
// the low-res cell nearest its centroid, then farthest-point samples (dlimgedit.h, DLIMG_STROKE_MARK).  map: width * height
// bytes of the segmentation's image, tightly packed; a pixel belongs to the stroke when its byte is >= 128.  label: 1, a
// foreground stroke drawn over the object, or 0, a background stroke over what the selection must leave out.  clicks: 1 .. 8;
// 0: the library's default, 3.  The sampled clicks count towards the 8 clicks of a prompt.  Travels as a stroke mark of table
// slot 14.
struct Stroke {
    uint8_t const* map = nullptr;
    int label = 1;
    int clicks = 0;
};

// A cut-out: the foreground colours of the image under a Matte's coverage, as RGBA (one pass of Blur-Fusion on the GPU, in
// integers; dlimgedit.h, DLIMG_CUTOUT_MARK), so that the object can be put on another background without a fringe of the old
// one.  rgba: receives height * width * 4 bytes, tightly packed -- the estimated foreground colour in the order of the guide's
// first three channels, then the coverage; it may be the Matte's guide itself when that has 4 channels (decontaminated in
// place).  radius: 1 .. 32 pixels; 0: the library's default, 16.  Needs a Matte of 3 or 4 channels on the same prompt; travels
// as a cut-out mark of table slot 14 directly behind the matte mark.  The mask the call returns is the coverage as ever.
struct Cutout {
    uint8_t* rgba = nullptr;
    int radius = 0;
};

// An edge mark: the mask a prompt delivers grown (offset > 0) or shrunk (offset < 0) by that many pixels with a disc, feathered by
// a linear ramp 2 * feather pixels wide, or turned into a band of `border` pixels on each side of the moved edge -- an editor's
// Select > Modify, by an exact Euclidean distance on the GPU, in integers (dlimgedit.h, DLIMG_EDGE_MARK).  offset -64 .. 64,
// feather 0 .. 32, border 0 .. 32, not all three 0.  A mask that touches the image's border is not shrunk from it.  Travels as an
// edge mark of table slot 14 behind the clean-up mark and in front of the matte mark, which then filters what this delivered.
struct Edge {
    int offset = 0;
    int feather = 0;
    int border = 0;
};

// One click of a click-to-refine prompt: on the object (foreground) or where the mask should not be (background).
struct Click {
    Point point;
    bool foreground = true;
};

// An encoded image (embedding resident in HBM) that answers mask queries cheaply.
class Segmentation {
  public:
    struct Mask {
        Image image;            // Channels::mask, values 0 / 255 (coverage 0 .. 255 from a prompt with a Matte)
        float accuracy = 0.0f;  // predicted IoU
    };

    static Segmentation process(ImageView const& image, Environment const& env) {
        Segmentation s(nullptr);
        dlimg_Segmentation h = nullptr;
        dlimg_Result r = api().process_image_for_segmentation(&h, reinterpret_cast<dlimg_ImageView const*>(&image), env.handle());
        s.handle_.reset(h);     // owned even when encoding failed
        detail::check(r);
        return s;
    }

    // Encodes several independent images in one batched pass (addition of this build).
    static std::vector<Segmentation> process_batch(std::vector<ImageView> const& images, Environment const& env) {
        std::vector<dlimg_Segmentation> hs(images.size(), nullptr);
        dlimg_Result r = api().process_images_for_segmentation(
            hs.data(), reinterpret_cast<dlimg_ImageView const*>(images.data()), int(images.size()), env.handle());
        std::vector<Segmentation> out;
        out.reserve(hs.size());
        for (auto h : hs) {
            out.emplace_back(nullptr);
            out.back().handle_.reset(h);
        }
        detail::check(r);
        return out;
    }

    void compute_mask(Point p, uint8_t* out_mask) const { query(&p.x, nullptr, out_mask); }
    void compute_mask(Region r, uint8_t* out_mask) const { query(nullptr, &r.top_left.x, out_mask); }
    Image compute_mask(Point p) const {
        Image m(extent(), Channels::mask);
        compute_mask(p, m.pixels());
        return m;
    }
    Image compute_mask(Region r) const {
        Image m(extent(), Channels::mask);
        compute_mask(r, m.pixels());
        return m;
    }

    // Three candidate masks for an ambiguous point, with their predicted accuracy.
    std::array<Mask, 3> compute_masks(Point p) const {
        std::array<Mask, 3> out{Mask{Image(extent(), Channels::mask)}, Mask{Image(extent(), Channels::mask)},
                                Mask{Image(extent(), Channels::mask)}};
        uint8_t* ptrs[3] = {out[0].image.pixels(), out[1].image.pixels(), out[2].image.pixels()};
        float acc[3] = {0, 0, 0};
        detail::check(api().get_segmentation_mask(handle_.get(), &p.x, nullptr, ptrs, acc));
        for (int i = 0; i < 3; ++i) out[i].accuracy = acc[i];
        return out;
    }

    // One single-mask query per segmentation, decoded as one batch (addition of this build): a point each, a region each
    // (points empty), or -- both given -- the region regions[i] refined by the foreground point points[i] in one prompt.
    static std::vector<Image> compute_mask_batch(std::vector<Segmentation const*> const& segs, std::vector<Point> const& points,
                                                 std::vector<Region> const& regions = {}) {
        if ((points.empty() && regions.empty()) || (!points.empty() && points.size() != segs.size()) ||
            (!regions.empty() && regions.size() != segs.size()))
            throw Exception("compute_mask_batch: one point and / or one region per segmentation");
        std::vector<dlimg_Segmentation> hs;
        std::vector<Image> out;
        std::vector<uint8_t*> ptrs;
        for (auto* s : segs) {
            hs.push_back(s->handle_.get());
            out.emplace_back(s->extent(), Channels::mask);
            ptrs.push_back(out.back().pixels());
        }
        static_assert(sizeof(Point) == 2 * sizeof(int) && sizeof(Region) == 4 * sizeof(int), "packed as the C table reads them");
        detail::check(api().get_segmentation_masks(hs.data(), int(hs.size()), points.empty() ? nullptr : &points.data()->x,
                                                   regions.empty() ? nullptr : &regions.data()->top_left.x, ptrs.data()));
        return out;
    }

    // Segment everything (addition of this build): a label map of the image, 0 where no segment lies and k in 1 .. 255 for
    // the k-th kept segment of a side x side point grid, the smallest segment on top (GridOptions; dlimgedit.h,
    // DLIMG_GRID_MARK).  Travels as a grid prompt of table slot 14: the head with an empty region, then the mark.
    void segment_everything(GridOptions const& grid, uint8_t* out_label_map) const {
        dlimg_Segmentation hs[2] = {handle_.get(), nullptr};
        const int regs[8] = {0, 0, -1, -1, DLIMG_GRID_MARK, grid.side, grid.iou_permille, grid.stability_permille};
        uint8_t* ptrs[2] = {out_label_map, nullptr};
        detail::check(api().get_segmentation_masks(hs, 2, nullptr, regs, ptrs));
    }
    Image segment_everything(GridOptions const& grid = {}) const {
        Image m(extent(), Channels::mask);
        segment_everything(grid, m.pixels());
        return m;
    }

    // Click-to-refine (addition of this build): one mask from 1 .. 8 clicks -- the first one a foreground click -- and an
    // optional box, as one prompt: the clicks in the order given, then the box.
    // refine_after: click counts k, strictly increasing, 1 <= k < clicks.size() -- "a refinement mark after the first k
    // clicks": the clicks are replayed in stages the way SAM's interactive predictor takes them, each stage with the low-res
    // logits of the one before it as its mask input (on the GPU); the mask of the last stage is returned.  refine_each(n):
    // a mark after every click but the last.  Needs a model with the mask branch.
    // clean: the mask is delivered cleaned (MaskCleanup).
    // prior: the caller's own mask as the mask input of the first stage (Prior).
    // lasso: the caller's selection, from which the box and / or the first click are derived (Lasso); the clicks given here
    // follow the derived one, and refine_after counts the clicks given here.  With DLIMG_LASSO_BOX there is no `region`.
    // matte: the mask is delivered as coverage 0 .. 255, its edge guided by the image (Matte), behind the clean-up.
    // strokes: scribbles whose sampled clicks follow the clicks given here (Stroke), in the order given; refine_after counts the
    // clicks given here.  (Behind matte, so that calls written before it read as they did.)
    // cutout: the image's foreground colours under the matte's coverage go to cutout->rgba (Cutout); needs matte.  (Behind
    // strokes, for the same reason.)
    // edge: the mask is grown, shrunk, feathered or bordered (Edge), behind the clean-up and in front of the matte.  (The last
    // argument, for the same reason.)
    Image compute_mask(std::vector<Click> const& clicks, std::optional<Region> region = std::nullopt,
                       std::vector<int> const& refine_after = {}, std::optional<MaskCleanup> clean = std::nullopt,
                       std::optional<Prior> prior = std::nullopt, std::optional<Lasso> lasso = std::nullopt,
                       std::optional<Matte> matte = std::nullopt, std::vector<Stroke> const& strokes = {},
                       std::optional<Cutout> cutout = std::nullopt, std::optional<Edge> edge = std::nullopt) const {
        return std::move(compute_mask_batch({this}, std::vector<std::vector<Click>>{clicks}, {region}, {refine_after},
                                            clean ? std::vector<std::optional<MaskCleanup>>{clean} : std::vector<std::optional<MaskCleanup>>{},
                                            prior ? std::vector<std::optional<Prior>>{prior} : std::vector<std::optional<Prior>>{},
                                            lasso ? std::vector<std::optional<Lasso>>{lasso} : std::vector<std::optional<Lasso>>{},
                                            matte ? std::vector<std::optional<Matte>>{matte} : std::vector<std::optional<Matte>>{},
                                            strokes.empty() ? std::vector<std::vector<Stroke>>{} : std::vector<std::vector<Stroke>>{strokes},
                                            cutout ? std::vector<std::optional<Cutout>>{cutout} : std::vector<std::optional<Cutout>>{},
                                            edge ? std::vector<std::optional<Edge>>{edge} : std::vector<std::optional<Edge>>{})[0]);
    }

    // Select by scribbling (addition of this build): the strokes alone are the prompt -- the clicks sampled from them in the
    // order given, the first FOREGROUND one first (so at least one stroke is a foreground stroke), and an optional box.  cleanup
    // matte, cutout and edge as for compute_mask.  out_mask may be a stroke's map itself.  A stroke without a pixel >= 128 is reported by the
    // library ("the stroke mark's map is empty") and nothing is delivered.
    void scribble(std::vector<Stroke> const& strokes, uint8_t* out_mask, std::optional<Region> region = std::nullopt,
                  std::optional<MaskCleanup> cleanup = std::nullopt, std::optional<Matte> matte = std::nullopt,
                  std::optional<Cutout> cutout = std::nullopt, std::optional<Edge> edge = std::nullopt) const {
        if (!out_mask) throw Exception("scribble: the result has a place to go");
        check_strokes(strokes, "scribble");
        check_matte(matte, "scribble");
        check_cutout(cutout, matte, "scribble");
        check_edge(edge, "scribble");
        if (cleanup && (cleanup->max_hole < 0 || cleanup->max_island < 0 || (cleanup->max_hole == 0 && cleanup->max_island == 0)))
            throw Exception("scribble: a clean-up mark has max_hole >= 0 and max_island >= 0, not both 0");
        if (std::none_of(strokes.begin(), strokes.end(), [](Stroke const& s) { return s.label == 1; }))
            throw Exception("scribble: background strokes alone are no prompt: one stroke is a foreground stroke");
        // the head with its box (or the empty region), the stroke marks, then the marks that stay last; no `points`
        std::vector<dlimg_Segmentation> hs{handle_.get()};
        std::vector<Region> regs{region ? *region : Region(Point{0, 0}, Point{-1, -1})};
        std::vector<uint8_t*> ptrs{out_mask};
        auto entry = [&](Region r, uint8_t const* read) {
            hs.push_back(nullptr);
            regs.push_back(r);
            ptrs.push_back(const_cast<uint8_t*>(read));          // a mark's out_masks pointer is only read
        };
        for (Stroke const& s : strokes) entry(Region(Point{DLIMG_STROKE_MARK, s.clicks}, Point{s.label, 0}), s.map);
        if (cleanup) entry(Region(Point{DLIMG_CLEAN_MARK, cleanup->max_hole}, Point{cleanup->max_island, 0}), nullptr);
        if (edge) entry(Region(Point{DLIMG_EDGE_MARK, edge->offset}, Point{edge->feather, edge->border}), nullptr);
        if (matte) entry(Region(Point{DLIMG_MATTE_MARK, matte->radius}, Point{matte->eps, matte->channels}), matte->guide);
        if (cutout) entry(Region(Point{DLIMG_CUTOUT_MARK, cutout->radius}, Point{0, 0}), cutout->rgba);     // (this one is written)
        detail::check(api().get_segmentation_masks(hs.data(), int(hs.size()), nullptr, &regs.data()->top_left.x, ptrs.data()));
    }
    Image scribble(std::vector<Stroke> const& strokes, std::optional<Region> region = std::nullopt,
                   std::optional<MaskCleanup> cleanup = std::nullopt, std::optional<Matte> matte = std::nullopt,
                   std::optional<Cutout> cutout = std::nullopt, std::optional<Edge> edge = std::nullopt) const {
        Image m(extent(), Channels::mask);
        scribble(strokes, m.pixels(), region, cleanup, matte, cutout, edge);
        return m;
    }
    static void check_strokes(std::vector<Stroke> const& strokes, char const* who) {
        int clicks = 0;
        for (Stroke const& s : strokes) {
            if (!s.map || (s.label != 0 && s.label != 1) || s.clicks < 0 || s.clicks > 8)
                throw Exception(std::string(who) + ": a stroke has a map, a label of 1 (foreground) or 0 (background) and 0 (the default, 3) .. 8 clicks");
            clicks += s.clicks ? s.clicks : 3;
        }
        if (strokes.empty() || clicks > 8) throw Exception(std::string(who) + ": strokes stand for 1 to 8 clicks in all");
    }

    // Snap a selection to the object (addition of this build): the lasso alone is the prompt -- its box, its most interior
    // point as a foreground click, and the selection itself as the mask input, whichever `what` names (Lasso) -- or the lasso
    // and further clicks behind the derived one.  refine_after, cleanup, matte, cutout and edge as for compute_mask.  out_mask may be
    // lasso.mask itself: a selection snapped in place.
    void snap(Lasso const& lasso, uint8_t* out_mask, std::vector<Click> const& clicks = {}, std::vector<int> const& refine_after = {},
              std::optional<MaskCleanup> cleanup = std::nullopt, std::optional<Matte> matte = std::nullopt,
              std::optional<Cutout> cutout = std::nullopt, std::optional<Edge> edge = std::nullopt) const {
        if (!lasso.mask || !out_mask) throw Exception("snap: a lasso has a mask, and the result a place to go");
        check_matte(matte, "snap");
        check_cutout(cutout, matte, "snap");
        check_edge(edge, "snap");
        if (cleanup && (cleanup->max_hole < 0 || cleanup->max_island < 0 || (cleanup->max_hole == 0 && cleanup->max_island == 0)))
            throw Exception("snap: a clean-up mark has max_hole >= 0 and max_island >= 0, not both 0");
        if (clicks.size() > 8) throw Exception("snap: a prompt takes at most 8 clicks");
        for (size_t m = 0; m < refine_after.size(); ++m)
            if (refine_after[m] < 1 || refine_after[m] >= int(clicks.size()) || (m && refine_after[m] <= refine_after[m - 1]))
                throw Exception("snap: refine_after holds click counts k, strictly increasing, 1 <= k < the clicks given");
        // the head with an empty region, the lasso mark directly behind it, then the further clicks and marks; without clicks
        // the call has no `points`, like a box-only call
        std::vector<dlimg_Segmentation> hs{handle_.get(), nullptr};
        std::vector<Point> pts{clicks.empty() ? Point{0, 0} : clicks[0].point, Point{0, 0}};
        std::vector<Region> regs{Region(Point{0, 0}, Point{-1, -1}), Region(Point{DLIMG_LASSO_MARK, lasso.strength_milli}, Point{lasso.what, 0})};
        std::vector<uint8_t*> ptrs{out_mask, const_cast<uint8_t*>(lasso.mask)};
        auto entry = [&](Point p, Region r) {
            hs.push_back(nullptr);
            pts.push_back(p);
            regs.push_back(r);
            ptrs.push_back(nullptr);
        };
        for (size_t c = 1; c < clicks.size(); ++c) {
            if (std::find(refine_after.begin(), refine_after.end(), int(c)) != refine_after.end())
                entry(Point{0, 0}, Region(Point{DLIMG_REFINE_MARK, 0}, Point{0, 0}));
            entry(clicks[c].point, Region(Point{clicks[c].foreground ? 1 : 0, 0}, Point{0, 0}));
        }
        if (!clicks.empty() && !clicks[0].foreground) throw Exception("snap: the first click given is a foreground click");
        if (cleanup) entry(Point{0, 0}, Region(Point{DLIMG_CLEAN_MARK, cleanup->max_hole}, Point{cleanup->max_island, 0}));
        if (edge) entry(Point{0, 0}, Region(Point{DLIMG_EDGE_MARK, edge->offset}, Point{edge->feather, edge->border}));
        if (matte) {
            entry(Point{0, 0}, Region(Point{DLIMG_MATTE_MARK, matte->radius}, Point{matte->eps, matte->channels}));
            ptrs.back() = const_cast<uint8_t*>(matte->guide);      // the mark's out_masks pointer is the guide, which the call only reads
        }
        if (cutout) {
            entry(Point{0, 0}, Region(Point{DLIMG_CUTOUT_MARK, cutout->radius}, Point{0, 0}));
            ptrs.back() = cutout->rgba;                            // the one mark whose out_masks pointer is written
        }
        detail::check(api().get_segmentation_masks(hs.data(), int(hs.size()), clicks.empty() ? nullptr : &pts.data()->x,
                                                   &regs.data()->top_left.x, ptrs.data()));
    }
    Image snap(Lasso const& lasso, std::vector<Click> const& clicks = {}, std::vector<int> const& refine_after = {},
               std::optional<MaskCleanup> cleanup = std::nullopt, std::optional<Matte> matte = std::nullopt,
               std::optional<Cutout> cutout = std::nullopt, std::optional<Edge> edge = std::nullopt) const {
        Image m(extent(), Channels::mask);
        snap(lasso, m.pixels(), clicks, refine_after, cleanup, matte, cutout, edge);
        return m;
    }
    static void check_matte(std::optional<Matte> const& m, char const* who) {
        if (m && (!m->guide || m->radius < 1 || m->radius > 32 || m->eps < 0 || m->eps > 65025 ||
                  (m->channels != 1 && m->channels != 3 && m->channels != 4)))
            throw Exception(std::string(who) + ": a matte has a guide, a radius of 1 .. 32, an eps of 0 (the default) .. 65025 and 1, 3 or 4 channels");
    }
    static void check_cutout(std::optional<Cutout> const& c, std::optional<Matte> const& m, char const* who) {
        if (c && (!c->rgba || c->radius < 0 || c->radius > 32 || !m || (m->channels != 3 && m->channels != 4)))
            throw Exception(std::string(who) + ": a cut-out has a place for its RGBA, a radius of 0 (the default) .. 32, and a matte of 3 or 4 channels on its prompt");
    }
    static void check_edge(std::optional<Edge> const& e, char const* who) {
        if (e && (e->offset < -64 || e->offset > 64 || e->feather < 0 || e->feather > 32 || e->border < 0 || e->border > 32 ||
                  (e->offset == 0 && e->feather == 0 && e->border == 0)))
            throw Exception(std::string(who) + ": an edge has an offset of -64 .. 64, a feather of 0 .. 32 and a border of 0 .. 32, not all three 0");
    }
    static std::vector<int> refine_each(size_t clicks) {
        std::vector<int> after;
        for (size_t k = 1; k < clicks; ++k) after.push_back(int(k));
        return after;
    }

    // The same for several segmentations in one batch; prompts of different sizes may share the call.  regions: empty, or one
    // optional box per prompt; refine_after: empty, or one list of marks per prompt (empty: none); clean: empty, or one
    // optional clean-up per prompt; prior: empty, or one optional prior per prompt; lasso: empty, or one optional lasso per
    // prompt (a prompt takes a prior or a lasso, not both); matte: empty, or one optional matte per prompt; strokes: empty, or
    // one list of strokes per prompt (empty: none), whose sampled clicks follow the prompt's clicks; cutout: empty, or one
    // optional cut-out per prompt (which then has a matte); edge: empty, or one optional edge per prompt.
    static std::vector<Image> compute_mask_batch(std::vector<Segmentation const*> const& segs,
                                                 std::vector<std::vector<Click>> const& clicks,
                                                 std::vector<std::optional<Region>> const& regions = {},
                                                 std::vector<std::vector<int>> const& refine_after = {},
                                                 std::vector<std::optional<MaskCleanup>> const& clean = {},
                                                 std::vector<std::optional<Prior>> const& prior = {},
                                                 std::vector<std::optional<Lasso>> const& lasso = {},
                                                 std::vector<std::optional<Matte>> const& matte = {},
                                                 std::vector<std::vector<Stroke>> const& strokes = {},
                                                 std::vector<std::optional<Cutout>> const& cutout = {},
                                                 std::vector<std::optional<Edge>> const& edge = {}) {
        if (clicks.size() != segs.size() || (!regions.empty() && regions.size() != segs.size()) ||
            (!refine_after.empty() && refine_after.size() != segs.size()) || (!clean.empty() && clean.size() != segs.size()) ||
            (!prior.empty() && prior.size() != segs.size()) || (!lasso.empty() && lasso.size() != segs.size()) ||
            (!matte.empty() && matte.size() != segs.size()) || (!strokes.empty() && strokes.size() != segs.size()) ||
            (!cutout.empty() && cutout.size() != segs.size()) || (!edge.empty() && edge.size() != segs.size()))
            throw Exception("compute_mask_batch: one list of clicks, at most one region and at most one list of marks per segmentation");
        for (auto const& p : prior)
            if (p && (!p->mask || p->strength_milli < 0 || p->strength_milli > 100000))
                throw Exception("compute_mask_batch: a prior has a mask and a strength_milli of 0 (the default) .. 100000");
        for (auto const& l : lasso)
            if (l && (!l->mask || l->what < 0 || l->what > 7 || l->what == DLIMG_LASSO_MASK || l->strength_milli < 0 || l->strength_milli > 100000))
                throw Exception("compute_mask_batch: a lasso has a mask, a `what` of 0 (all) .. 7 other than 4, and a strength_milli of 0 .. 100000");
        for (auto const& m : matte) check_matte(m, "compute_mask_batch");
        for (size_t j = 0; j < cutout.size(); ++j)
            check_cutout(cutout[j], matte.empty() ? std::optional<Matte>{} : matte[j], "compute_mask_batch");
        for (auto const& e : edge) check_edge(e, "compute_mask_batch");
        for (auto const& s : strokes)
            if (!s.empty()) check_strokes(s, "compute_mask_batch");
        for (auto const& c : clean)
            if (c && (c->max_hole < 0 || c->max_island < 0 || (c->max_hole == 0 && c->max_island == 0)))
                throw Exception("compute_mask_batch: a clean-up mark has max_hole >= 0 and max_island >= 0, not both 0");
        for (size_t j = 0; j < refine_after.size(); ++j)
            for (size_t m = 0; m < refine_after[j].size(); ++m)
                if (refine_after[j][m] < 1 || refine_after[j][m] >= int(clicks[j].size()) || (m && refine_after[j][m] <= refine_after[j][m - 1]))
                    throw Exception("compute_mask_batch: refine_after holds click counts k, strictly increasing, 1 <= k < the prompt's clicks");
        std::vector<Image> out;
        bool refined = false;
        for (size_t j = 0; j < segs.size(); ++j) {
            if (clicks[j].empty() || clicks[j].size() > 8) throw Exception("compute_mask_batch: a prompt takes 1 to 8 clicks");
            if (!clicks[j][0].foreground) throw Exception("compute_mask_batch: the first click of a prompt is a foreground click");
            refined = refined || clicks[j].size() > 1 || (!clean.empty() && clean[j].has_value()) ||
                      (!prior.empty() && prior[j].has_value()) || (!lasso.empty() && lasso[j].has_value()) ||
                      (!matte.empty() && matte[j].has_value()) || (!strokes.empty() && !strokes[j].empty()) ||
                      (!edge.empty() && edge[j].has_value());                                                  // any continuation entry
            out.emplace_back(segs[j]->extent(), Channels::mask);
        }
        // The entry lists of table slot 14: the head entry of a prompt carries the handle, the first click and the box (an
        // empty region, x1 < x0: none); every further click is an entry without a handle whose region holds its label.
        // Without any further click the entries are plain point and box + point entries, where an empty region means nothing
        // special: then the prompts without a box go in a call without regions, the others in one with both arrays.
        for (int pass = 0; pass < (refined ? 1 : 2); ++pass) {
            std::vector<dlimg_Segmentation> hs;
            std::vector<Point> pts;
            std::vector<Region> regs;
            std::vector<uint8_t*> ptrs;
            for (size_t j = 0; j < segs.size(); ++j) {
                const bool box = !regions.empty() && regions[j].has_value();
                if (!refined && box != (pass == 1)) continue;
                for (size_t c = 0; c < clicks[j].size(); ++c) {
                    if (!refine_after.empty() && std::find(refine_after[j].begin(), refine_after[j].end(), int(c)) != refine_after[j].end()) {
                        hs.push_back(nullptr);           // a mark after the first c clicks: its point is not read
                        pts.push_back(Point{0, 0});
                        ptrs.push_back(nullptr);
                        regs.push_back(Region(Point{DLIMG_REFINE_MARK, 0}, Point{0, 0}));
                    }
                    hs.push_back(c == 0 ? segs[j]->handle_.get() : nullptr);
                    pts.push_back(clicks[j][c].point);
                    ptrs.push_back(c == 0 ? out[j].pixels() : nullptr);
                    if (c == 0) regs.push_back(box ? *regions[j] : Region(Point{0, 0}, Point{-1, -1}));
                    else regs.push_back(Region(Point{clicks[j][c].foreground ? 1 : 0, 0}, Point{0, 0}));
                    if (c == 0 && !prior.empty() && prior[j]) {
                        hs.push_back(nullptr);           // the prior mark, directly behind its head: its point is not read and
                        pts.push_back(Point{0, 0});      // its out_masks pointer is the prior, which the call only reads
                        ptrs.push_back(const_cast<uint8_t*>(prior[j]->mask));
                        regs.push_back(Region(Point{DLIMG_PRIOR_MARK, prior[j]->strength_milli}, Point{0, 0}));
                    }
                    if (c == 0 && !lasso.empty() && lasso[j]) {
                        hs.push_back(nullptr);           // the lasso mark, directly behind its head, likewise: its out_masks pointer
                        pts.push_back(Point{0, 0});      // is the selection
                        ptrs.push_back(const_cast<uint8_t*>(lasso[j]->mask));
                        regs.push_back(Region(Point{DLIMG_LASSO_MARK, lasso[j]->strength_milli}, Point{lasso[j]->what, 0}));
                    }
                }
                if (!strokes.empty())
                    for (Stroke const& s : strokes[j]) {
                        hs.push_back(nullptr);           // a stroke mark, behind the clicks given: its point is not read and its
                        pts.push_back(Point{0, 0});      // out_masks pointer is the map, which the call only reads
                        ptrs.push_back(const_cast<uint8_t*>(s.map));
                        regs.push_back(Region(Point{DLIMG_STROKE_MARK, s.clicks}, Point{s.label, 0}));
                    }
                if (!clean.empty() && clean[j]) {
                    hs.push_back(nullptr);               // the clean-up mark, the last entry of its prompt: its point is not read
                    pts.push_back(Point{0, 0});
                    ptrs.push_back(nullptr);
                    regs.push_back(Region(Point{DLIMG_CLEAN_MARK, clean[j]->max_hole}, Point{clean[j]->max_island, 0}));
                }
                if (!edge.empty() && edge[j]) {
                    hs.push_back(nullptr);               // the edge mark, behind the clean-up mark and in front of the matte mark:
                    pts.push_back(Point{0, 0});          // neither its point nor its pointer is read
                    ptrs.push_back(nullptr);
                    regs.push_back(Region(Point{DLIMG_EDGE_MARK, edge[j]->offset}, Point{edge[j]->feather, edge[j]->border}));
                }
                if (!matte.empty() && matte[j]) {
                    hs.push_back(nullptr);               // the matte mark, behind everything else of its prompt: its point is not
                    pts.push_back(Point{0, 0});          // read and its out_masks pointer is the guide, which the call only reads
                    ptrs.push_back(const_cast<uint8_t*>(matte[j]->guide));
                    regs.push_back(Region(Point{DLIMG_MATTE_MARK, matte[j]->radius}, Point{matte[j]->eps, matte[j]->channels}));
                }
                if (!cutout.empty() && cutout[j]) {
                    hs.push_back(nullptr);               // the cut-out mark, directly behind the matte mark: its point is not read
                    pts.push_back(Point{0, 0});          // and its out_masks pointer is WRITTEN, the RGBA
                    ptrs.push_back(cutout[j]->rgba);
                    regs.push_back(Region(Point{DLIMG_CUTOUT_MARK, cutout[j]->radius}, Point{0, 0}));
                }
            }
            if (hs.empty()) continue;
            detail::check(api().get_segmentation_masks(hs.data(), int(hs.size()), &pts.data()->x,
                                                       (refined || pass == 1) ? &regs.data()->top_left.x : nullptr, ptrs.data()));
        }
        return out;
    }

    Extent extent() const noexcept {
        Extent e;
        api().get_segmentation_extent(handle_.get(), &e.width);
        return e;
    }

    Segmentation(std::nullptr_t) noexcept {}
    dlimg_Segmentation handle() const noexcept { return handle_.get(); }
    explicit operator bool() const noexcept { return bool(handle_); }

  private:
    void query(int const* point, int const* region, uint8_t* out_mask) const {
        uint8_t* ptrs[3] = {out_mask, nullptr, nullptr};   // second slot null selects single-mask mode
        float acc[3] = {0, 0, 0};
        detail::check(api().get_segmentation_mask(handle_.get(), point, region, ptrs, acc));
    }
    std::unique_ptr<dlimg_Segmentation_, detail::SegDeleter> handle_;
};
static_assert(sizeof(Point) == 8 && sizeof(Region) == 16 && sizeof(Extent) == 8, "POD layouts of the C-ABI");

// Dichotomous foreground segmentation (BiRefNet in the reference): reported as unsupported by this build.
inline void segment_objects(ImageView const& image, uint8_t* out_mask, Environment const& env) {
    detail::check(api().segment_objects(reinterpret_cast<dlimg_ImageView const*>(&image), out_mask, env.handle()));
}
inline Image segment_objects(ImageView const& image, Environment const& env) {
    Image m(image.extent, Channels::mask);
    segment_objects(image, m.pixels(), env);
    return m;
}

}  // namespace dlimg
