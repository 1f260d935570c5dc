// p2varcoefsteps.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// The schedule of the fused steps of the two P2 variable-coefficient operators (P2ElementwiseDivKGrad, P2ViscousBlockEpsilonOperator):
// residual, Jacobi step, Chebyshev start and Chebyshev step through hyteg_hip_p2_elementwise_{divkgrad,epsilon}_*_cell, written once over
// NC components.  An operator hands in how it applies itself on the shell classes and how it calls the C-ABI entry of a mode on one cell.
//   * A storage with one macro-cell: every DoF is complete on the cell -- one fused call with the full masks, nothing is exchanged.
//   * Several macro-cells (sharesInnerShell of p1epsilon.hpp): this cell's shares of A src on the shell classes by the Replace apply
//     restricted to HYTEG_HIP_MASK_SHELL, the fused call on HYTEG_HIP_MASK_INNER, the additive exchange of the shares, then the mode's
//     vector passes on the shell only (keep = HYTEG_HIP_MASK_SHELL, vertex and edge DoFs alike), per component under that component's own
//     condition.  Components with different boundary conditions stay on this path: the kernels take a class mask per component.  The
//     exchange is not split around the inner call (sharesInnerShell overlaps the first one): it runs after it.
#pragma once

#include "p2function.hpp"

namespace hyteg {
namespace p2varcoef {

enum class Step
{
   Residual,  // out = rhs - A src
   Jacobi,    // out = src + a inv ( rhs - A src )                      a = relax
   ChebStart, // out = inv ( rhs - A src ); on the shell also x += a out   a = c0 (src is x; elsewhere the update is deferred)
   ChebStep   // out = inv A src; x = ( x + cPrev src ) + a out            a = cCur (on the shell x += a out: cPrev was applied there)
};

template < size_t NC >
struct Operands
{
   std::array< const P2Function< double >*, NC > out, src, rhs, inv, x; // null where the step has none
};

// the classes the fused call covers, and the classes left to the shell passes
inline unsigned fusedClasses( const PrimitiveStorage& storage ) { return storage.getCells().size() > 1 ? HYTEG_HIP_MASK_INNER : HYTEG_HIP_MASK_ALL; }

// shellApply(): out = A src (Replace) on HYTEG_HIP_MASK_SHELL; cell( c, masks ): the C-ABI entry of the step on local cell c
template < size_t NC, class ShellApply, class Cell >
void fusedStep( const std::shared_ptr< PrimitiveStorage >& storage, Step step, const Operands< NC >& f, const std::array< Selection, NC >& flag,
                uint_t level, double a, ShellApply&& shellApply, Cell&& cell )
{
   const bool     shared  = storage->getCells().size() > 1;
   const unsigned classes = fusedClasses( *storage );
   if ( shared )
      shellApply();
   std::array< std::vector< unsigned >, NC > masks;
   for ( size_t k = 0; k < NC; ++k )
      masks[k] = storage->masksFor( flag[k], false, classes );
   for ( uint_t c = 0; c < storage->getNumberOfLocalCells(); ++c )
   {
      std::array< unsigned, NC > m;
      unsigned                   any = 0;
      for ( size_t k = 0; k < NC; ++k )
         any |= m[k] = masks[k][c];
      if ( any )
         cell( c, m );
   }
   if ( !shared )
      return;
   constexpr unsigned S = HYTEG_HIP_MASK_SHELL;
   for ( size_t k = 0; k < NC; ++k )
   {
      const P2Function< double >& out = *f.out[k];
      out.getVertexDoFFunction().sumSharedCopies( level, flag[k] );
      out.sumSharedEdgeCopies( level, flag[k] );
      if ( step != Step::ChebStep )
         out.assignKinds( { 1.0, -1.0 }, { *f.rhs[k], out }, level, flag[k], 0xFFu, S );
      if ( step != Step::Residual )
         out.multElementwiseKinds( { *f.inv[k], out }, level, flag[k], 0xFFu, S );
      if ( step == Step::Jacobi )
         out.assignKinds( { 1.0, a }, { *f.src[k], out }, level, flag[k], 0xFFu, S );
      if ( step == Step::ChebStart || step == Step::ChebStep )
         f.x[k]->assignKinds( { 1.0, a }, { *f.x[k], out }, level, flag[k], 0xFFu, S );
   }
}

// x += c t where the fused start deferred it: closes a smoother call of order 1
template < size_t NC >
void chebyshevFinish( const std::shared_ptr< PrimitiveStorage >& storage, const std::array< const P2Function< double >*, NC >& x,
                      const std::array< const P2Function< double >*, NC >& t, const std::array< Selection, NC >& flag, double c, uint_t level )
{
   for ( size_t k = 0; k < NC; ++k )
      x[k]->assignKinds( { 1.0, c }, { *x[k], *t[k] }, level, flag[k], 0xFFu, fusedClasses( *storage ) );
}

} // namespace p2varcoef
} // namespace hyteg
