// Image extents, prompt coordinates and the longest-side-to-1024 geometry: pure host code (no HIP, no environment), so that
// the prompt packer of prompt_plan.hpp is tested without a GPU.
#pragma once

#include <algorithm>

namespace dlimg {

struct Extent { int width = 0, height = 0; };
struct Point { int x = 0, y = 0; };
struct Region { Point top_left, bottom_right; };

constexpr int kPromptFrame = 1024;        // the encoder's image size (sam_model.hpp: kImageSize)

inline int scale_coord(int coord, float scale) { return int(float(coord) * scale + 0.5f); }       // reference: segmentation.cpp:26

// Longest-side-to-1024 geometry (reference: segmentation.cpp:58-74).  The pixel resampling itself is
// a device kernel here; this struct only keeps the numbers needed later for prompts and masks.
struct ResizeLongestSide {
    Extent original;
    Extent resized;
    float scale = 1.f;

    explicit ResizeLongestSide(int max_side = kPromptFrame) : max_side_(max_side) {}
    void set(Extent image) {
        original = image;
        scale = float(max_side_) / float(std::max(image.width, image.height));
        resized = image;
        if (scale != 1) resized = Extent{scale_coord(image.width, scale), scale_coord(image.height, scale)};
    }
    Point transform(Point p) const { return Point{scale_coord(p.x, scale), scale_coord(p.y, scale)}; }

  private:
    int max_side_;
};

}  // namespace dlimg
