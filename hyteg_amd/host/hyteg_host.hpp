// hyteg_host.hpp -- C++ host layer above the C-ABI (include/hyteg_hip.h).
//
// Mirrors the names and call signatures of the reference classes on the P1 hot path so that code written
// against HyTeG reads the same here:
//   MeshInfo                     src/hyteg/mesh/MeshInfo.hpp:221,512-585
//   PrimitiveStorage             src/hyteg/primitivestorage/PrimitiveStorage.hpp, SetupPrimitiveStorage.cpp
//   BoundaryCondition, BoundaryUID   src/hyteg/boundary/BoundaryConditions.hpp
//   P1Function< double >         src/hyteg/p1functionspace/VertexDoFFunction.hpp/.cpp (interpolate, assign, add,
//                                multElementwise, dotLocal, dotGlobal)
//   P1ConstantOperator< Form >   src/constant_stencil_operator/P1ConstantOperator.hpp:33-168 + P1Operator.hpp:192-447
//   operatorgeneration::P1ElementwiseDiffusion, P1ElementwiseDivKGrad   module hyteg_operators (generated classes)
//   P1ElementwiseAffineEpsilonOperator, P1P1ElementwiseAffineEpsilonStokesOperator   src/mixed_operator/P1EpsilonOperator.hpp,
//                                P1P1ElementwiseAffineEpsilonStokesOperator.hpp (viscosity: a P1Function)
//   P1toP1LinearRestriction / P1toP1LinearProlongation   src/hyteg/gridtransferoperators/
//   P1toP2Conversion / P2toP1Conversion, P1toP1QuadraticProlongationThroughP2Injection           src/hyteg/gridtransferoperators/
//   WeightedJacobiSmoother, GaussSeidelSmoother, SORSmoother, CGSolver, GeometricMultigridSolver,
//   FullMultigridSolver                                                                           src/hyteg/solvers/
//   P1ProjectNormalOperator, StrongFreeSlipWrapper   src/hyteg/p1functionspace/P1ProjectNormalOperator.hpp, src/hyteg/composites/StrongFreeSlipWrapper.hpp
//   ChebyshevSmoother, chebyshev::estimateRadius, InvDiagOperatorWrapper                         src/hyteg/solvers/ChebyshevSmoother.hpp
//
// Data model: one device array per (macro-cell, level) in HyTeG's cell layout.  The DoFs
// of macro-faces/edges/vertices are the boundary entries of every adjacent cell array and are kept bit-identical
// in all copies.  Operators evaluate them as per-cell partial results + one additive exchange ("sumShared"),
// which is what HyTeG itself does for elementwise operators and grid transfer
// (P1ElementwiseOperator.cpp:186-188, P1toP1LinearRestriction.cpp:343-345), instead of the six directed ghost
// phases of P1Operator.hpp:201-207.  All device work goes through the C-ABI; this file launches nothing itself.
#pragma once
#pragma once

#include "types.hpp"
#include "boundary.hpp"
#include "mesh.hpp"
#include "storage.hpp"
#include "p1function.hpp"
#include "p2function.hpp"
#include "forms.hpp"
#include "p1operator.hpp"
#include "p1elementwise.hpp"
#include "p1divkgrad.hpp"
#include "p2operator.hpp"
#include "p2divkgrad.hpp"
#include "p2gridtransfer.hpp"
#include "gridtransfer.hpp"
#include "p1p2conversion.hpp"
#include "solvers.hpp"
#include "chebyshev.hpp"
#include "stokes.hpp"
#include "p1epsilon.hpp"
#include "taylorhood.hpp"
#include "p2epsilon.hpp"
#include "projectnormal.hpp"
