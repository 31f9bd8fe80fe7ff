// Measurements of the point-to-line and point-to-plane pose edges (ref: src/measurements.h).  Plain host
// structures: the optimiser flattens them (icp_types.h).  Member names and constructors are the reference's.
#pragma once
#include <cmath>

#include "cugo_types.h"

namespace cugo
{

/** a point matched to an infinite line through a and b (all in the frame the pose estimate maps into) */
template <typename S>
class PointToLineMatch
{
public:
    Vec3d a, b; // two points of the line (start, end)
    S length{}; // |b - a| as the constructor computed it; the optimiser recomputes direction and length from a, b
    Vec3d pointP; // the matched point, in platform coordinates

    PointToLineMatch() {}
    PointToLineMatch(const Vec3d& start, const Vec3d& finish) : a(start), b(finish)
    {
        const S dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
        length = std::sqrt(dx * dx + dy * dy + dz * dz);
    }
    Vec3d start() const { return a; }
    Vec3d end() const { return b; }
};

/** a point matched to the plane {x : normal . x = originDistance} */
template <typename S>
class PointToPlaneMatch
{
public:
    PointToPlaneMatch() {}
    /** norm: unit normal (used as given), offset: signed distance of the plane from the origin */
    PointToPlaneMatch(const Vec3d& norm, S offset, const Vec3d& point) : normal(norm), originDistance(offset), pointP(point)
    {
    }

    Vec3d normal;
    S originDistance{};
    Vec3d pointP;
};

} // namespace cugo
