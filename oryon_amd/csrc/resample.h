// The bilinear tap of the K-1 resizes (preproc.hip, augment.hip): torch's upsample_bilinear2d with align_corners=False.
//   src = scale*(dst+0.5)-0.5 clamped at 0, i0 = floor(src), i1 = i0 + (i0 < in-1), l1 = src-i0, l0 = 1-l1.
#pragma once

namespace oryon {

template <typename T>
struct Tap { int i0, i1; T l0, l1; };

template <typename T>
__device__ __forceinline__ Tap<T> make_tap(int dst, T scale, int in_size)
{
    T src = scale * ((T)dst + (T)0.5) - (T)0.5;
    src = src < (T)0 ? (T)0 : src;
    Tap<T> t;
    t.i0 = (int)src;
    if (t.i0 > in_size - 1) t.i0 = in_size - 1;
    t.i1 = t.i0 + (t.i0 < in_size - 1 ? 1 : 0);
    t.l1 = src - (T)t.i0;
    t.l0 = (T)1 - t.l1;
    return t;
}

}  // namespace oryon
